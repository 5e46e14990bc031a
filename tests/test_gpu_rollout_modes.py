"""`Rollout.modes`, `GNN.modes` and `GNN.evaluate(modes=)` on the tiny synthetic meshes of the other rollout tests: the modes of a rollout
are those of `Modes.fit` on its own step-major buffer and on its `result()`, bit for bit; a renumbered rollout gives the same mean and
modes in the caller's rows up to the order of summation; only the slots of steps taken are read; and a rollout that does not ask for
modes allocates and launches what it did — the three launches run when `modes()` is called, never in `__init__` or `step()`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import modes_ref as R                                      # noqa: E402
import graphs4cfd_amd as gfd                               # noqa: E402
from graphs4cfd_amd import _lib, ops, synthetic as S       # noqa: E402
from graphs4cfd_amd.nn.model import Rollout                # noqa: E402

DEV = torch.device("cuda", 0)
N_OUT, NF = 7, 3
LAUNCHES = ("g4c_snapshot_mean", "g4c_snapshot_gram", "g4c_snapshot_combine")


@pytest.fixture(scope="module")
def mesh():
    g = S.mus_graph(3000, levels=3, seed=3).to(DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(4)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    target = torch.randn(g.num_nodes, NF * N_OUT + 2, generator=torch.Generator().manual_seed(5)).to(DEV)
    full = model.solve(g.clone(), N_OUT)
    gen = torch.Generator().manual_seed(6)
    nw = torch.rand(g.num_nodes, generator=gen, dtype=torch.float64) + 0.5
    return dict(g=g, model=model, target=target, full=full, nw=nw, fw=torch.tensor([1.0, 2.0, 0.0], dtype=torch.float64))


def same(a, b, what):
    """Two SnapshotModes hold the same bits."""
    for name in ("gram", "mean", "modes", "singular_values", "energy", "coefficients"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or torch.equal(x, y), f"{what}: {name}"
    assert a.dropped == b.dropped
    if a.dmd is not None or b.dmd is not None:
        assert torch.equal(a.dmd.gram, b.dmd.gram), f"{what}: dmd.gram"
        # (the same Gram matrix; a non-symmetric eigenproblem is not asked to give the same bits twice)
        assert torch.allclose(a.dmd.eigenvalues, b.dmd.eigenvalues, rtol=1e-9, atol=1e-9) and a.dmd.modes.shape == b.dmd.modes.shape, f"{what}: dmd"


def ones_tol(m):
    """How far from one the cosines of a subspace with itself may be: the eigen-decomposition leaves V Sigma^2 V^T within M 2^-52 lambda_0
    of the Gram matrix, and Sigma^-1 V^T G V Sigma^-1 divides that by the smallest eigenvalue kept."""
    s = m.singular_values
    return 64 * m.gram.size(0) * 2.0 ** -52 * float(s[0] / s[-1]) ** 2


def steps_of(result, nf=NF):
    """[N, nf M] -> the step-major [M, N, nf]."""
    return result.reshape(result.size(0), -1, nf).permute(1, 0, 2).contiguous()


def test_rollout_modes_are_fit_on_its_own_buffer(mesh):
    spec = gfd.Modes(node_weights=mesh["nw"], field_weights=mesh["fw"], dmd=True, dt=0.1)
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False) as ro:
        ro.run(N_OUT)
        got, res = ro.modes(spec), ro.result()
        same(got, spec.fit(ro._out_steps), "fit on _out_steps")
    assert torch.equal(res, mesh["full"])
    cols = spec.fit(res, layout="columns")
    assert torch.equal(cols.gram, got.gram) and torch.equal(cols.mean, got.mean)
    same(got, cols, "fit on result()")
    M, n = N_OUT, mesh["g"].num_nodes
    assert tuple(got.gram.shape) == (M, M) and tuple(got.mean.shape) == (n, NF) and tuple(got.modes.shape[1:]) == (n, NF)
    assert got.modes.size(0) == got.singular_values.numel() <= M - 1 and got.dropped >= 1 and got.modes.is_cuda and got.gram.device.type == "cpu"
    # against the restatement: the mean bit for bit, the Gram matrix within its bound, the modes orthonormal
    flat = steps_of(res).cpu().numpy().reshape(M, -1)
    w = (mesh["nw"][:, None] * mesh["fw"][None, :]).reshape(-1).numpy()
    R.same_bits(got.mean.reshape(-1), R.mean(flat), "mean")
    ref, Sabs = R.gram(flat, mean_a=R.mean(flat), w=w)
    assert (np.abs(got.gram.numpy() - ref) <= 2.0 * (flat.shape[1] + 4) * 2.0 ** -53 * Sabs).all()
    modes = got.modes.cpu().numpy().reshape(got.modes.size(0), -1).astype(np.float64)
    orth = np.abs((modes * w) @ modes.T - np.eye(modes.shape[0])).max()
    print("orthonormality of a rollout's modes:", orth, "allowed", 16 * M * 2.0 ** -24)
    assert orth <= 16 * M * 2.0 ** -24
    assert float(got.modes[:, :, 2].abs().max()) > 0          # (a field left out of the inner product still has its mode shape)
    assert np.abs(got.alignment(got).numpy() - 1.0).max() <= ones_tol(got)
    assert got.dmd.modes.dtype == torch.complex64 and got.dmd.frequency.numel() == got.dmd.eigenvalues.numel()


def test_every_start_and_stride(mesh):
    spec = gfd.Modes(start=1, stride=2, count=2, centre=False)
    with Rollout(mesh["model"], mesh["g"], 13, reorder=False, every=3) as ro:
        ro.run(13)
        got, res = ro.modes(spec), ro.result()
        assert tuple(ro._out_steps.shape[:1]) == (4,)
        with pytest.raises(ValueError, match="^count:"):
            ro.modes(gfd.Modes(count=5))
    assert tuple(got.gram.shape) == (2, 2) and got.mean is None
    kept = steps_of(res)                                       # slots 0 .. 3: steps 2, 5, 8, 11
    same(got, gfd.Modes(centre=False).fit(kept[1::2].contiguous()), "slots 1 and 3")
    ref, _ = R.gram(kept.cpu().numpy().reshape(4, -1), sel_a=(1, 2, 2))
    assert np.abs(got.gram.numpy() - ref).max() <= 1e-12 * np.abs(ref).max()


def test_only_the_slots_of_steps_taken(mesh):
    g, f0 = mesh["g"], mesh["g"].field
    try:
        with Rollout(mesh["model"], g, N_OUT, reorder=False) as ro:
            ro.run(3)
            three = ro.modes(gfd.Modes())
            assert tuple(three.gram.shape) == (3, 3)
            same(three, gfd.Modes().fit(ro._out_steps[:3].clone()), "three steps taken")
            with pytest.raises(ValueError, match="^count:"):
                ro.modes(gfd.Modes(count=4))
            ro.run(2)
            ro.rewind()                                        # the device step index is 1 again: slot 0 is kept, slots 1 .. are stale
            one = ro.modes(gfd.Modes(centre=False))
            assert tuple(one.gram.shape) == (1, 1)
            with pytest.raises(ValueError, match="^start:"):
                ro.modes(gfd.Modes(start=1))
            ro.run(2)
            after = ro.modes(gfd.Modes())
            assert tuple(after.gram.shape) == (3, 3)
            same(after, gfd.Modes().fit(ro._out_steps[:3].clone()), "after rewind")
    finally:
        g.field = f0


def test_every_zero_raises(mesh):
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, every=0, target=mesh["target"]) as ro:
        ro.run(2)
        with pytest.raises(RuntimeError, match="every=0"):
            ro.modes(gfd.Modes())
        with pytest.raises(TypeError, match="^modes:"):
            ro.modes(dict(rank=2))


def test_renumbered_rollout_gives_the_callers_rows(mesh):
    """reorder=True forced: the rollout's rows are Morton-ordered, the node weights go through the permutation, and mean and modes come
    back in the caller's rows — compared with a fit on the same rollout's `result()`, which is in the caller's rows throughout.  The
    mean is bit for bit (one thread per column: a column's sum keeps its order); the Gram matrix has the same terms in another order."""
    spec = gfd.Modes(rank=2, node_weights=mesh["nw"], field_weights=mesh["fw"])
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=True) as ro:
        ro.run(N_OUT)
        assert ro._perm is not None
        moved, res = ro.modes(spec), ro.result()
    plain = spec.fit(res, layout="columns")
    assert torch.equal(moved.mean, plain.mean)
    flat = steps_of(res).cpu().numpy().reshape(N_OUT, -1)
    w = (mesh["nw"][:, None] * mesh["fw"][None, :]).reshape(-1).numpy()
    R.same_bits(moved.mean.reshape(-1), R.mean(flat), "mean")
    ref, Sabs = R.gram(flat, mean_a=R.mean(flat), w=w)
    bound = 2.0 * (flat.shape[1] + 4) * 2.0 ** -53 * Sabs
    assert (np.abs(moved.gram.numpy() - ref) <= bound).all() and (np.abs(plain.gram.numpy() - ref) <= bound).all()
    # what a perturbation of the Gram matrix within its bound does to V / sigma, to a cosine and to a coefficient: at most its norm over
    # the smallest eigenvalue kept (the two kept are far apart) — far below the fp32 rounding the modes are stored with
    lam = float(moved.singular_values[-1]) ** 2
    tol = 8.0 * N_OUT * float(bound.max()) / lam + 64 * 2.0 ** -52
    print("renumbered: Gram bound over the smallest kept eigenvalue", tol)
    assert float((moved.modes - plain.modes).abs().max()) <= (4 * 2.0 ** -24 + tol) * float(plain.modes.abs().max())
    assert np.abs(moved.alignment(plain).numpy() - 1.0).max() <= tol and np.abs(plain.alignment(moved).numpy() - 1.0).max() <= tol
    assert np.abs(moved.project(steps_of(res)).numpy() - moved.coefficients.numpy()).max() <= tol * float(moved.singular_values[0])


def test_a_rollout_without_modes_is_what_it_was(mesh, monkeypatch):
    """A spy on the library's entry points: `__init__` and `step()` never call the three launches; `modes()` does."""
    lib = _lib.load()
    calls = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name not in LAUNCHES:
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped
    monkeypatch.setattr(_lib, "load", lambda: Spy())
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False) as ro:
        ro.run(N_OUT)
        plain = ro.result().clone()
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False) as ro:
        ro.run(N_OUT)
        assert calls == []
        ro.modes(gfd.Modes(dmd=True))
        assert calls == ["g4c_snapshot_mean", "g4c_snapshot_gram", "g4c_snapshot_gram"] + ["g4c_snapshot_combine"] * 3
        with_modes = ro.result()
    assert torch.equal(with_modes, plain) and torch.equal(plain, mesh["full"])


def test_gnn_modes_and_evaluate(mesh):
    g, model, full = mesh["g"].clone(), mesh["model"], mesh["full"]
    g.target = mesh["target"][:, :NF * N_OUT].contiguous()
    got = model.modes(g.clone(), N_OUT, rank=2, dmd=True)
    assert type(got) is gfd.SnapshotModes and got.modes.size(0) == 2
    same(got, gfd.Modes(rank=2, dmd=True).fit(full, layout="columns", nf=NF), "GNN.modes")
    same(got, model.modes(g.clone(), N_OUT, gfd.Modes(rank=2, dmd=True), capture=False), "GNN.modes(spec)")
    strided = model.modes(g.clone(), N_OUT, every=2, centre=False)
    same(strided, gfd.Modes(centre=False).fit(steps_of(full)[1::2].contiguous()), "every=2")
    errs = model.evaluate(g.clone())
    assert errs.modes is None
    spec = gfd.Modes(rank=3)
    both = model.evaluate(g.clone(), every=1, modes=spec)
    assert torch.equal(both.sums, errs.sums)
    same(both.modes.prediction, spec.fit(full, layout="columns", nf=NF), "evaluate, prediction")
    same(both.modes.target, spec.fit(g.target, layout="columns", nf=NF), "evaluate, target")
    assert tuple(both.modes.alignment.shape) == (3,) and bool((both.modes.alignment <= 1 + 1e-12).all())
    assert np.abs(both.modes.target.alignment(both.modes.target).numpy() - 1.0).max() <= ones_tol(both.modes.target)
    assert torch.equal(both.modes.alignment, both.modes.prediction.alignment(both.modes.target))
    two = model.evaluate(g.clone(), every=2, modes=gfd.Modes(rank=2))      # the target's columns of the kept steps 1, 3, 5
    same(two.modes.target, gfd.Modes(rank=2).fit(steps_of(g.target)[1::2].contiguous()), "evaluate every=2, target")


def test_list_of_two_graphs():
    graphs = [S.mus_graph(n, levels=1, seed=20 + n).to(DEV) for n in (300, 500)]
    torch.manual_seed(9)
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 64), device=DEV)
    full = model.solve([gr.clone() for gr in graphs], N_OUT)
    got = model.modes([gr.clone() for gr in graphs], N_OUT, rank=2)
    assert tuple(got.modes.shape) == (2, 800, NF)
    same(got, gfd.Modes(rank=2).fit(full, layout="columns", nf=NF), "two graphs")
