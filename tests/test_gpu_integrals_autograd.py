"""`ControlVolumes.integrate` under autograd (autograd._WeightedIntegrals), `per_graph=` and `ControlVolumes.adjoint`: the recorded call
returns the unrecorded call's bits, `.backward()` leaves exactly `adjoint(g, ...)` in `.grad`, row q of `per_graph=True` is a
single-graph `ControlVolumes`' result bit for bit, the gradient agrees with torch's own autograd of Σ area · z_a · z_b in fp64 within the
restatement's bound (tests/integrals_adjoint_ref.py), two runs are bit-identical, and a `sub` that requires a gradient is refused."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import integrals_adjoint_ref as A          # noqa: E402
import voronoi_ref as V                    # noqa: E402
import graphs4cfd_amd as gfd               # noqa: E402

DEV = torch.device("cuda", 0)
ENTRIES = [(0, 0), (1, 1), (0, 1), (2, -1), (-1, -1), (-1, 0)]
COUNTS = (257, 300)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def graph_of(pos, batch=None):
    g = gfd.Graph()
    g.pos = dev(pos)
    if batch is not None:
        g.batch = dev(batch)
    return g


@pytest.fixture(scope="module")
def world():
    """The volumes of a batch of two overlapping graphs, of each graph alone, and fixed fields (never modified)."""
    p = [V.uniform_cloud(COUNTS[0]), V.jittered_lattice(COUNTS[1], seed=2)]
    batch = np.concatenate([np.full(c, q, np.int64) for q, c in enumerate(COUNTS)])
    both = gfd.ControlVolumes(graph_of(np.concatenate(p), batch=batch))
    alone = [gfd.ControlVolumes(graph_of(q)) for q in p]
    gen = torch.Generator().manual_seed(3)
    n = sum(COUNTS)
    x = torch.randn((n, 4), generator=gen).to(DEV)
    sub = torch.randn((n, 5), generator=gen).to(DEV)
    return dict(both=both, alone=alone, x=x, sub=sub, n=n)


def bits(t):
    return t.detach().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def test_counts_and_group(world):
    cv = world["both"]
    assert cv.counts == list(COUNTS)
    assert cv.group.dtype == torch.int32 and cv.group.device == cv.area.device
    assert torch.equal(cv.group.cpu(), torch.repeat_interleave(torch.arange(2, dtype=torch.int32), torch.tensor(COUNTS)))
    assert world["alone"][0].counts == [COUNTS[0]] and not bool(world["alone"][0].group.any())


@pytest.mark.parametrize("with_sub", [False, True])
def test_per_graph_rows_are_the_single_graphs_bits(world, with_sub):
    cv, x = world["both"], world["x"]
    sub = world["sub"] if with_sub else None
    rows = cv.integrate(x, ENTRIES, sub=sub, nz=3, per_graph=True)
    assert tuple(rows.shape) == (2, len(ENTRIES)) and rows.dtype == torch.float64
    a = 0
    for q, c in enumerate(COUNTS):
        one = world["alone"][q].integrate(x[a:a + c].contiguous(), ENTRIES, sub=None if sub is None else sub[a:a + c].contiguous(), nz=3)
        assert torch.equal(bits(rows[q]), bits(one)), q
        a += c
    whole = cv.integrate(x, ENTRIES, sub=sub, nz=3)
    assert tuple(whole.shape) == (len(ENTRIES),)
    assert torch.allclose(whole, rows.sum(0), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("per_graph", [False, True])
@pytest.mark.parametrize("with_sub", [False, True])
def test_the_recorded_call_and_its_backward(world, per_graph, with_sub):
    cv = world["both"]
    sub = world["sub"] if with_sub else None
    plain = cv.integrate(world["x"], ENTRIES, sub=sub, nz=3, per_graph=per_graph)
    x = world["x"].clone().requires_grad_(True)
    out = cv.integrate(x, ENTRIES, sub=sub, nz=3, per_graph=per_graph)
    assert out.requires_grad and torch.equal(bits(out), bits(plain))
    with torch.no_grad():
        assert not cv.integrate(x, ENTRIES, sub=sub, nz=3, per_graph=per_graph).requires_grad
    g = torch.randn(out.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(DEV)
    out.backward(g)
    gx = cv.adjoint(g, world["x"], ENTRIES, sub=sub, nz=3, per_graph=per_graph)
    assert tuple(gx.shape) == (world["n"], 3) and gx.dtype == torch.float32
    assert tuple(x.grad.shape) == tuple(x.shape)
    assert torch.equal(bits(x.grad[:, :3]), bits(gx))
    assert not bool(bits(x.grad[:, 3:]).any())          # the column beside the sample: +0
    # two runs: the same bits
    x2 = world["x"].clone().requires_grad_(True)
    cv.integrate(x2, ENTRIES, sub=sub, nz=3, per_graph=per_graph).backward(g)
    assert torch.equal(bits(x2.grad), bits(x.grad))
    # the restatement's bits, and torch's own autograd of the same sums in fp64 within the restatement's bound
    group = cv.group.cpu().numpy() if per_graph else None
    acc, addends = A.adjoint64(world["x"].cpu().numpy(), cv.area.cpu().numpy(), ENTRIES, g.cpu().numpy().reshape(-1, len(ENTRIES)),
                               None if sub is None else sub.cpu().numpy(), group=group, nz=3)
    assert np.array_equal(gx.cpu().numpy().view(np.int32), A.cast(acc).view(np.int32))
    z = world["x"][:, :3].double().clone().requires_grad_(True)
    zz = z if sub is None else z - sub[:, :3].double()
    one = torch.ones(world["n"], dtype=torch.float64, device=DEV)
    T = torch.stack([cv.area * (one if a < 0 else zz[:, a]) * (one if b < 0 else zz[:, b]) for a, b in ENTRIES], dim=1)       # [N, ne]
    if per_graph:
        I = torch.stack([T[cv.group == q].sum(0) for q in range(2)])
    else:
        I = T.sum(0)
    (I * g).sum().backward()
    err = (gx.double() - z.grad).abs().cpu().numpy()
    bound = A.bound(acc, addends, len(ENTRIES))
    print(f"per_graph={per_graph} sub={with_sub}: largest |gx − autograd| / bound = {(err / np.maximum(bound, 1e-300)).max():.3e}")
    assert (err <= bound).all()


def test_a_strided_target_source_is_differentiated_at_its_step(world):
    cv = world["both"]
    x = world["x"].clone().requires_grad_(True)          # two steps of two columns
    out = cv.integrate(x, [(0, 1), (1, 1)], x_step=2, t=1)
    assert torch.equal(bits(out), bits(cv.integrate(world["x"][:, 2:4].contiguous(), [(0, 1), (1, 1)])))
    g = torch.tensor([2.0, -3.0], dtype=torch.float64, device=DEV)
    out.backward(g)
    want = cv.adjoint(g, world["x"][:, 2:4].contiguous(), [(0, 1), (1, 1)])
    assert torch.equal(bits(x.grad[:, 2:4]), bits(want)) and not bool(bits(x.grad[:, :2]).any())


def test_a_sub_that_requires_grad_is_refused(world):
    cv = world["both"]
    x = world["x"].clone().requires_grad_(True)
    sub = world["sub"].clone().requires_grad_(True)
    with pytest.raises(ValueError, match="^sub:"):
        cv.integrate(x, ENTRIES, sub=sub, nz=3)
    with pytest.raises(ValueError, match="^sub:"):
        cv.integrate(world["x"], ENTRIES, sub=sub, nz=3)
    with torch.no_grad():
        cv.integrate(world["x"], ENTRIES, sub=sub, nz=3)
    with pytest.raises(ValueError, match="^g:"):
        cv.adjoint(torch.zeros(3, dtype=torch.float64, device=DEV), world["x"], ENTRIES, nz=3)
    with pytest.raises(ValueError, match="^per_graph:"):
        cv.integrate(world["x"], ENTRIES, nz=3, per_graph=1)
