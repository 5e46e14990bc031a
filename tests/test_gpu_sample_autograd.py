"""`gfd.PointSampler.sample` under autograd: of an x that requires grad the sample is recorded — the same launch, the same bits — and its
backward is the adjoint launch (`g4c_sample_points_adjoint`), bit for bit `PointSampler.adjoint`, for the dense, the stride-0 and the
column-sliced gradients autograd hands over; without grad nothing changes.  (Before the sampler was differentiable the result had no
`grad_fn`: a loss on sampled values trained nothing.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import sample_adjoint_ref as A                           # noqa: E402
import sampler_ref as SR                                 # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402

DEV = torch.device("cuda", 0)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sampler_of(dim):
    pos = SR.cloud(300, dim)
    pts = SR.queries(257, dim)
    return gfd.PointSampler(gfd.Graph(pos=dev(pos)), dev(pts)), 300, 257


@pytest.mark.parametrize("dim", [2, 3])
def test_sample_is_recorded_and_its_backward_is_the_adjoint(dim):
    s, n, n_points = sampler_of(dim)
    x0 = dev(np.random.default_rng(3).standard_normal((n, 3)).astype(np.float32))
    plain = s.sample(x0)
    assert plain.grad_fn is None and not plain.requires_grad and s._adjoint_tables is None
    x = x0.clone().requires_grad_(True)
    with torch.no_grad():          # nothing changes: no grad_fn, out= is taken, the same bits
        out = torch.empty(n_points, 3, device=DEV)
        quiet = s.sample(x, out=out)
        assert quiet is out and quiet.grad_fn is None and torch.equal(bits(quiet), bits(plain)) and s._adjoint_tables is None
    y = s.sample(x)
    assert y.grad_fn is not None and y.requires_grad and torch.equal(bits(y), bits(plain))          # the same launch: the same bits
    with pytest.raises(NotImplementedError, match="out="):
        s.sample(x, out=torch.empty(n_points, 3, device=DEV))
    # a dense gy
    gy = dev(A.gy_of(n_points, 3))
    (gx,) = torch.autograd.grad(y, x, gy, retain_graph=True)
    assert torch.equal(bits(gx), bits(s.adjoint(gy)))
    # .sum(): autograd hands over a stride-0 expanded tensor of ones
    (gx,) = torch.autograd.grad(y.sum(), x, retain_graph=True)
    assert torch.equal(bits(gx), bits(s.adjoint(torch.ones(n_points, 3, device=DEV))))
    # a column slice: a dense gy that is zero outside the slice
    w = dev(np.random.default_rng(4).standard_normal((n_points, 1)).astype(np.float32))
    (gx,) = torch.autograd.grad((y[:, 1:2] * w).sum(), x, retain_graph=True)
    full = torch.zeros(n_points, 3, device=DEV)
    full[:, 1:2] = w
    assert torch.equal(bits(gx), bits(s.adjoint(full))) and not bits(gx[:, [0, 2]]).any() and bool(gx[:, 1].any())
    # a strided x (a column slice of a wider tensor: rows of unit stride) is sampled and differentiated as well
    wide = torch.zeros(n, 5, device=DEV)
    wide[:, 1:4] = x0
    wide.requires_grad_(True)
    ys = s.sample(wide[:, 1:4])
    assert torch.equal(bits(ys), bits(plain))
    (gw,) = torch.autograd.grad(ys, wide, gy)
    assert torch.equal(bits(gw[:, 1:4]), bits(s.adjoint(gy))) and not bits(gw[:, [0, 4]]).any()
    with pytest.raises(RuntimeError):          # once_differentiable: no double backward
        (g1,) = torch.autograd.grad(s.sample(x).sum(), x, create_graph=True)
        g1.sum().backward()


@pytest.mark.parametrize("dim", [2, 3])
def test_the_dot_product_identity_on_the_device(dim):
    """⟨S x, y⟩ = ⟨x, ∂⟨S x, y⟩/∂x⟩ within the forward's and the adjoint's fp32 bounds (tests/sampler_ref.py, tests/sample_adjoint_ref.py)."""
    s, n, n_points = sampler_of(dim)
    rng = np.random.default_rng(9)
    xs, ys = rng.standard_normal((n, 4)).astype(np.float32), rng.standard_normal((n_points, 4)).astype(np.float32)
    x = dev(xs).requires_grad_(True)
    fwd = s.sample(x)
    (gx,) = torch.autograd.grad(fwd, x, dev(ys))
    idx, coef = s._idx.cpu().numpy(), s._coef.cpu().numpy()
    mag = SR.apply64(xs, idx.T, coef.T)[1]
    bound = A.adjoint64(ys, *A.node_tables(idx, coef, n))[1]
    lhs = float((fwd.detach().cpu().numpy().astype(np.float64) * ys).sum())
    rhs = float((xs.astype(np.float64) * gx.cpu().numpy().astype(np.float64)).sum())
    allowed = float((SR.bound32(mag, s.k) * np.abs(ys)).sum() + (bound * np.abs(xs)).sum()) * (1 + 1e-6)
    assert abs(lhs - rhs) <= allowed, (lhs, rhs, allowed)
    assert abs(lhs) > 1e2 * allowed          # (the check has teeth)
