"""`gfd.BodyForces.forces` and `.wall` of an x that requires grad are recorded for autograd: the values are the plain launch's bits, the
backward is `BodyForces.adjoint`'s bits for a dense, a stride-0 and a column-sliced incoming gradient; under `no_grad`, and for an x
that does not require grad, the path is the plain one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import forces_ref as FR                                  # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import synthetic as S                # noqa: E402

DEV = torch.device("cuda", 0)
I32, I64 = torch.int32, torch.int64
SCALE, SHIFT, MU = [1.5, 0.75, 2.5, 1.0], [0.25, -0.5, 0.125, 0.0], 0.03125 * 1.3
_cache = {}


def bits(t):
    return t.detach().contiguous().view(I64 if t.dtype == torch.float64 else I32)


def setup():
    if not _cache:
        pos, wall, label = FR.annulus(300, (37, 5), seed=2)
        g = gfd.Graph(pos=torch.from_numpy(pos).to(DEV))
        g.edge_index = S.connect_knn(g.pos, 6)[0]
        kw = dict(nodes=torch.from_numpy(wall).to(DEV), bodies=torch.from_numpy(label).to(DEV), scale=SCALE, shift=SHIFT)
        _cache.update(n=len(pos), visc=gfd.BodyForces(g, mu=MU, **kw), inviscid=gfd.BodyForces(g, **kw),
                      x=torch.randn(len(pos), 4, generator=torch.Generator().manual_seed(1)).to(DEV))
    return _cache


@pytest.mark.parametrize("which", ["visc", "inviscid"])
def test_forces_and_wall_are_recorded(which):
    c = setup()
    op, x = c[which], c["x"]
    plain_f, plain_w = op.forces(x), op.wall(x)
    assert plain_f.grad_fn is None and plain_w.grad_fn is None and not plain_f.requires_grad
    xr = x.clone().requires_grad_(True)
    f, w = op.forces(xr), op.wall(xr)
    assert f.grad_fn is not None and w.grad_fn is not None                 # (no grad_fn before the adjoint existed: a loss trained nothing)
    assert f.dtype == torch.float64 and torch.equal(bits(f), bits(plain_f)) and torch.equal(bits(w), bits(plain_w))
    gen = torch.Generator().manual_seed(4)
    gF, gw = torch.randn(op.n_bodies, 6, generator=gen, dtype=torch.float64).to(DEV), torch.randn(op.n_items, 2, generator=gen).to(DEV)
    # a dense gradient
    (a,) = torch.autograd.grad(f, xr, gF, retain_graph=True)
    (b,) = torch.autograd.grad(w, xr, gw, retain_graph=True)
    assert tuple(a.shape) == tuple(x.shape) and a.dtype == torch.float32
    assert torch.equal(bits(a), bits(op.adjoint(gF, None, nf=4))) and torch.equal(bits(b), bits(op.adjoint(None, gw, nf=4)))
    assert not a[:, 3].view(I32).any()                                    # a column the operator does not read: +0
    # stride 0: what .sum().backward() hands over
    (a,) = torch.autograd.grad(f.sum(), xr, retain_graph=True)
    (b,) = torch.autograd.grad(w.sum(), xr, retain_graph=True)
    assert torch.equal(bits(a), bits(op.adjoint(torch.ones_like(gF), None, nf=4))) and torch.equal(bits(b), bits(op.adjoint(None, torch.ones_like(gw), nf=4)))
    # a column slice: the drag alone, the surface pressure alone
    (a,) = torch.autograd.grad((f[:, 0] + f[:, 2]).sum(), xr, retain_graph=True)
    only = torch.zeros_like(gF)
    only[:, [0, 2]] = 1.0
    assert torch.equal(bits(a), bits(op.adjoint(only, None, nf=4)))
    (b,) = torch.autograd.grad((w[:, 0] * gw[:, 0]).sum(), xr, retain_graph=True)
    only = torch.zeros_like(gw)
    only[:, 0] = gw[:, 0]
    assert torch.equal(bits(b), bits(op.adjoint(None, only, nf=4)))
    # both through one backward: autograd adds the two adjoints
    xr.grad = None
    ((f * gF).sum().to(torch.float32) + (w * gw).sum()).backward()
    assert torch.isfinite(xr.grad).all() and xr.grad.abs().sum() > 0
    if which == "inviscid":
        assert not xr.grad[:, [0, 1, 3]].any()                            # mu == 0: only the pressure column


def test_no_grad_and_plain_inputs_take_the_plain_path():
    c = setup()
    op, x = c["visc"], c["x"]
    fresh = gfd.BodyForces.__new__(gfd.BodyForces)
    fresh.__dict__.update(op.__dict__)
    fresh._adjoint_tables = None
    xr = x.clone().requires_grad_(True)
    with torch.no_grad():
        f, w = fresh.forces(xr), fresh.wall(xr)
    assert f.grad_fn is None and w.grad_fn is None and not f.requires_grad and not w.requires_grad
    assert torch.equal(bits(f), bits(op.forces(x))) and torch.equal(bits(w), bits(op.wall(x)))
    h = fresh.history(torch.cat([xr, xr], 1), 2, nf=4)                     # not differentiable, as before
    assert h.grad_fn is None and torch.equal(bits(h[1]), bits(f))
    assert fresh._adjoint_tables is None                                   # nothing of the adjoint was built
    f, w = fresh.forces(x), fresh.wall(x)                                  # grad enabled, a plain x
    assert f.grad_fn is None and w.grad_fn is None and fresh._adjoint_tables is None
