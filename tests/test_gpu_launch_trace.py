"""The launches of the MP-layer host path, row for row: which `g4c_mlp_run` / `g4c_segment_reduce` calls a forward issues, in which
order, with which host-visible arguments, and which kernel the launcher chose for each (tests/launch_trace.py records them).  The code
that decides this — nn/blocks.py, the three models, partition.py — may be rearranged; the launches may not change with it.

tests/golden/launch_traces.json was recorded from the Python package of commit 2543cc0 (the host path before its decisions were each
given one place) with this tree's library, by `scripts/mp_host_path.py record` — not read off the code under test, and not to be
regenerated after an edit to that code: a row that changes is a changed launch.

Cases (launch_trace.case_ids; sizes on either side of HOIST_MIN_ROWS 24 576, RS1_MIN_ROWS / the weight-stationary threshold 20 000,
FUSE_LAYER_MIN_ROWS 2 048, and where a route needs it ops.FUSE_AGG_MIN_ROWS / AGG_ON_LOAD_MIN_ROWS 50 000 and FUSE_LAYER_MAX_ROWS 120 000):
  mus-{300,1000,5000}-{f16x3,bf16x6,bf16,fp32}   NsTwoScaleGNN, k = 6, bare forward() under no_grad
  mus-20000-f16x3-rollout2                       the same model, Rollout(capture=False), two steps: an active StaticCache
  mus-1000-f16x3-grad                            gradients enabled, forward + backward
  remus-{246,984}-{bf16,f16x3}, remus-4000-bf16  NsRotEquiTreeScaleGNN, k = 5: 984 nodes are the fewest with 24 576 level-1 angle rows
  mugs-5000-f16x3                                NsTwoGuillardScaleGNN: 2H-wide latents behind the up-sampling
  part-mus-17200-f16x3-overlap{1,0}, part-remus-984-bf16    world 2, the ranks as threads (partition_harness.run_ranks)
ROUTES says which case reaches which route; the golden must hold a row of every one."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import launch_trace as LT                                                      # noqa: E402
from graphs4cfd_amd import _lib                                                # noqa: E402

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_traces.json")) as _f:
    GOLDEN = json.load(_f)["cases"]


def _src(r, pred):
    return r["call"] == "mlp" and any(pred(s) for s in r["sources"])


# route -> (a row of it, the case that reaches it)
ROUTES = {
    "two fp32 heads": (lambda r: r["call"] == "mlp" and r["n_heads"] == 2 and r["head_dtype"] == 0, "mus-5000-f16x3"),
    "bf16 heads": (lambda r: r["call"] == "mlp" and r["n_heads"] > 0 and r["head_dtype"] == 1, "remus-984-bf16"),
    "mlp_rs1_kernel": (lambda r: r["call"] == "mlp" and r["last_kernel"] == _lib.KERNEL_MLP_RS, "remus-984-bf16"),
    "mlp_rs2_kernel": (lambda r: r["call"] == "mlp" and r["last_kernel"] == _lib.KERNEL_MLP_RS2, "remus-4000-bf16"),
    "the fused layer (upd)": (lambda r: r["call"] == "mlp" and r["upd"], "mus-1000-f16x3"),
    "mlp_ws_pre_kernel": (lambda r: r["call"] == "mlp" and r["last_kernel"] == _lib.KERNEL_MLP_WS_PRE, "mus-20000-f16x3-rollout2"),
    "aggregation on load (seg_off)": (lambda r: _src(r, lambda s: s["seg_off"]), "part-mus-17200-f16x3-overlap1"),
    "aggregate without rows (keep_e=False)": (lambda r: r["call"] == "mlp" and r["agg"] and not r["out"], "mus-20000-f16x3-rollout2"),
    "products of a separate launch": (lambda r: _src(r, lambda s: s["additive"] and s["idx"] and s["from_product_launch"]), "mus-5000-f16x3"),
    "a reduction behind an MLP launch": (lambda r: r["call"] == "reduce" and r["behind_mlp"], "mus-5000-fp32"),
    "saved rows (n_save > 0)": (lambda r: r["call"] == "mlp" and r["n_save"] > 0, "mus-1000-f16x3-grad"),
}


def _rows(case):
    return [LT.as_dict(r) for rows in GOLDEN[case].values() for r in rows]


def test_golden_holds_the_cases_and_every_route():
    assert list(GOLDEN) == LT.case_ids()
    for route, (pred, case) in ROUTES.items():
        assert any(pred(r) for r in _rows(case)), f"no row of the route '{route}' in the golden trace of {case}"


@pytest.mark.parametrize("case", list(GOLDEN))
def test_trace_equals_the_parents(case):
    with LT.LaunchTrace() as rows:
        out = LT.run(case)
    assert all(bool(torch.isfinite(t).all()) for t in out.values())
    got = json.loads(json.dumps(rows))          # (tuples -> lists, as the golden went through JSON)
    want = GOLDEN[case]
    assert sorted(got) == sorted(want), f"threads that launched: {sorted(got)}, recorded: {sorted(want)}"
    for who in want:
        for i, (g, w) in enumerate(zip(got[who], want[who])):
            assert g == w, f"{case} {who} launch {i}:\n  now      {LT.as_dict(g)}\n  recorded {LT.as_dict(w)}"
        assert len(got[who]) == len(want[who]), f"{case} {who}: {len(got[who])} launches, recorded {len(want[who])}"
