"""Test-only whole-mesh references of the partitioned step (graphs4cfd_amd/partition.py, partition_remus.py), stage by stage.

Every stage of MusPartitionedForward / RemusPartitionedForward is restated once on the WHOLE mesh, as a composition of
oracle/g4c_oracle.py (`mlp`, `scatter`, `down_mp` with its `pool_edge`, `up_mp`, `down_edge_mp`, `edge_scalar_to_node_vector`,
`knn_interpolate`), and evaluated in whatever dtype / device its inputs have: float64 is the reference, float32 on the device is the
comparator of fwd_ref.assert_as_accurate_as_fp32.  The first-layer product heads are W1[:, a:b] y.

Stage-local (the rule of tests/test_gpu_fwd_ref.py): a stage's reference starts from the tensors the ranks themselves stored for
the stages before it, assembled into whole-mesh order (`rec`, from tests/partition_harness.py) — and inside an MP layer the node
update starts from the layer's own stored messages.  A wrong row then is an O(1) error at its own stage instead of diluted noise at
the end.  Nothing here knows about ranks, halos or local numbering: that is the point.

Perturbations (negative controls, on a reference only): `wrong_boundary_sender`, `rows_moved`."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import g4c_oracle as O

Tensor = torch.Tensor
SFX = {1: "", 2: "2", 3: "3"}


def cast(d: Dict[str, Tensor], dtype, device) -> Dict[str, Tensor]:
    """Floating tensors in `dtype`, everything on `device` (a graph dict, a state dict, one stage's recorded tensors)."""
    return {k: (v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device)) if torch.is_tensor(v) else v for k, v in d.items()}


def cast_rec(rec, dtype, device):
    return {key: cast(ent, dtype, device) for key, ent in rec.items()}


def _act(x: Tensor, pending: bool) -> Tensor:
    return F.selu(x) if pending else x


def product_heads(y: Tensor, w, next_name: str) -> Tuple[Tensor, Tensor]:
    """(W1r y, W1c y) of the first layer of `next_name`'s message MLP: W1 = [W1e | W1r | W1c] over [e | v_row | v_col]."""
    H = int(y.size(1))
    W1 = w[f"{next_name}.edge_mlp.MLP.linear_1.weight"]
    return y @ W1[:, -2 * H:-H].t(), y @ W1[:, -H:].t()


def mlp_after_first(h: Tensor, w, prefix: str) -> Tensor:
    """O.mlp from behind its first Linear (whose bias is already in h): (SELU, Linear)*, LayerNorm."""
    n = 1
    while f"{prefix}.MLP.linear_{n + 1}.weight" in w:
        n += 1
    for i in range(2, n + 1):
        h = F.linear(F.selu(h), w[f"{prefix}.MLP.linear_{i}.weight"], w[f"{prefix}.MLP.linear_{i}.bias"])
    g = w.get(f"{prefix}.MLP.layer_norm.weight")
    return h if g is None else F.layer_norm(h, (h.size(-1),), g, w[f"{prefix}.MLP.layer_norm.bias"], 1e-5)


# ------------------------------------------------------------------------------------- MuS-GNN
def mus_stages(model: str, g: Dict[str, Tensor], w, rec, nf: int, edges: Dict[int, Tensor], had_products: Dict[int, bool],
               only: Optional[Sequence[int]] = None, check_topology: bool = True):
    """{(position, stage): {name: whole-mesh reference}} with the keys and names of partition_harness.assemble_mus.
    `edges[level]`: the level's global edge list (partition.coarse_topology); `had_products[k]`: MP layer k took its node-side
    first-layer terms as products (then its messages are restated from them, as the layer computes them).  `only`: positions to
    evaluate (the walk over the program still follows every stage's recorded outputs)."""
    prog = O.MUS_PROGRAMS[model]
    want = (lambda k: True) if only is None else (lambda k: k in set(only))
    out = {}
    R = rec[(-1, "encode")]
    if want(-1):
        x = torch.cat([g[k] for k in ("field", "loc", "glob", "omega") if k in g], 1)
        o = {"e": F.selu(O.mlp(g["edge_attr"], w, "edge_encoder")), "v": F.selu(O.mlp(x, w, "node_encoder"))}
        if "prod_r" in R:
            o["prod_r"], o["prod_c"] = product_heads(R["v"], w, prog[0][1])
        out[(-1, "encode")] = o
    v, e, pending, level, stash = R["v"], R["e"], False, 1, []
    prod = (R["prod_r"], R["prod_c"]) if "prod_r" in R else None
    for k, op in enumerate(prog):
        R = rec[(k, op[0])]
        if op[0] == "mp":
            name = op[1]
            if want(k):
                row, col = edges[level][0], edges[level][1]
                ea = _act(e, pending)
                if had_products[k]:
                    H = int(v.size(1))
                    W1, b1 = w[f"{name}.edge_mlp.MLP.linear_1.weight"], w[f"{name}.edge_mlp.MLP.linear_1.bias"]
                    e_new = mlp_after_first(ea @ W1[:, :-2 * H].t() + prod[0][row] + prod[1][col] + b1, w, f"{name}.edge_mlp")
                else:
                    e_new = O.mlp(torch.cat((ea, v[row], v[col]), 1), w, f"{name}.edge_mlp")
                agg = O.scatter(R["e"], col, int(v.size(0)), "mean")
                o = {"e": e_new, "v": F.selu(O.mlp(torch.cat((agg, v), 1), w, f"{name}.node_mlp"))}
                if "prod_r" in R:
                    o["prod_r"], o["prod_c"] = product_heads(R["v"], w, prog[k + 1][1])
                out[(k, "mp")] = o
            v, e, pending = R["v"], R["e"], True
            prod = (R["prod_r"], R["prod_c"]) if "prod_r" in R else None
        elif op[0] == "down":
            if want(k):
                v_c, ei_c, e_c = O.down_mp(g, v, edges[level], _act(e, pending), w, op[1], level, torch.tanh)
                if check_topology:
                    assert torch.equal(ei_c, edges[level + 1]), "the oracle's pool_edge and partition.coarse_topology order the coarse edges alike"
                out[(k, "down")] = {"v_c": v_c, "e_pool": e_c}
            stash.append((v, e, pending))
            v, e, pending, prod, level = R["v_c"], R["e_pool"], False, None, level + 1
        else:
            v_old, e_old, p_old = stash.pop()
            if want(k):
                o = {"v": O.up_mp(g, v, v_old, w, op[1], level, torch.tanh)}
                if "prod_r" in R:
                    o["prod_r"], o["prod_c"] = product_heads(R["v"], w, prog[k + 1][1])
                out[(k, "up")] = o
            v, e, pending, level = R["v"], e_old, p_old, level - 1
            prod = (R["prod_r"], R["prod_c"]) if "prod_r" in R else None
    if want(len(prog)):
        out[(len(prog), "decode")] = {"pred": g["field"][:, -nf:] + O.mlp(v, w, "node_decoder")}
    return out


# ------------------------------------------------------------------------------------- REMuS-GNN
def _project(v: Tensor, col: Tensor, unit: Tensor) -> Tensor:
    return (v[col].reshape(col.size(0), -1, 2) * unit.unsqueeze(1)).sum(-1)


def remus_stages(g: Dict[str, Tensor], w, rec, program, only: Optional[Sequence[int]] = None, raw_angles: bool = True):
    """{(position, stage): {name: whole-mesh reference}} with the keys and names of partition_harness.assemble_remus; `program` is
    NsRotEquiTreeScaleGNN._PROGRAM ((op, module, level) with op in mp / down / up).  `raw_angles`: an EdgeMP stores its angle
    latents WITHOUT the activation (RemusHipImpl: the next reader applies it while loading, and the edge update starts from the
    stored rows); False: it stores them activated (the oracle back-end of the CPU tests; the edge update then starts from the
    reference's own raw rows)."""
    want = (lambda k: True) if only is None else (lambda k: k in set(only))
    out = {}
    if want(-1):
        o = {}
        for l, s in SFX.items():
            col = g[f"edge_index{s}"][1]
            x = torch.cat([_project(g["field"], col, g[f"edgeUnitVector{s}"]), g["glob"][col], g["omega"][col]], 1)
            o[f"e{l}"] = F.selu(O.mlp(x, w, f"edge_encoder{s}"))
            o[f"a{l}"] = F.selu(O.mlp(g[f"angle_attr{s}"], w, f"angle_encoder{s}"))
        o["ax1"] = F.selu(O.mlp(g["angle_attr12"], w, "angle_encoder12"))
        o["ax2"] = F.selu(O.mlp(g["angle_attr23"], w, "angle_encoder23"))
        out[(-1, "encode")] = o
    R = rec[(-1, "encode")]
    e = {l: R[f"e{l}"] for l in SFX}
    a = {l: R[f"a{l}"] for l in SFX}
    ax = {1: R["ax1"], 2: R["ax2"]}
    a_pending = {l: False for l in SFX}
    for k, (op, name, lvl) in enumerate(program):
        if op == "mp":
            R = rec[(k, "mp")]
            if want(k):
                row, col = g[f"angle_index{SFX[lvl]}"][0], g[f"angle_index{SFX[lvl]}"][1]
                a_new = O.mlp(torch.cat((_act(a[lvl], a_pending[lvl]), e[lvl][row], e[lvl][col]), 1), w, f"{name}.angle_mlp")
                agg = O.scatter(R["a"] if raw_angles else a_new, col, int(e[lvl].size(0)), "mean")
                out[(k, "mp")] = {"a": a_new if raw_angles else F.selu(a_new), "e": F.selu(O.mlp(torch.cat((agg, e[lvl]), 1), w, f"{name}.edge_mlp"))}
            e[lvl], a[lvl], a_pending[lvl] = R["e"], R["a"], raw_angles
        elif op == "down":
            R = rec[(k, "down")]
            if want(k):
                out[(k, "down")] = {"e": F.selu(O.down_edge_mp(e[lvl], e[lvl + 1], ax[lvl], g[f"angle_index{lvl}{lvl + 1}"], w, name))}
            e[lvl + 1] = R["e"]
        else:
            lo, hi = lvl, lvl - 1
            Rn, Ru = rec[(k, "node_vectors")], rec[(k, "up")]
            if want(k):
                out[(k, "node_vectors")] = {"n": O.edge_scalar_to_node_vector(e[lo], g[f"edge_index{SFX[lo]}"], unit_inv=g[f"edgeUnitVectorInverse{SFX[lo]}"],
                                                                              coarse_mask=g[f"coarse_mask{lo}"])}
                nb = Rn["n"]
                v1 = nb.new_zeros(int(g["pos"].size(0)), int(nb.size(1)))
                interp = O.knn_interpolate(nb, g[f"y_idx_{lo}{hi}"], g[f"x_idx_{lo}{hi}"], g[f"weights_{lo}{hi}"])
                if hi == 1:
                    v1 = interp
                else:
                    v1[g[f"coarse_mask{hi}"]] = interp
                proj = _project(v1, g[f"edge_index{SFX[hi]}"][1], g[f"edgeUnitVector{SFX[hi]}"])
                out[(k, "up")] = {"e": F.selu(O.mlp(torch.cat((proj, e[hi]), 1), w, f"{name}.up_mlp"))}
            e[hi] = Ru["e"]
    if want(len(program)):
        s = O.mlp(e[1], w, "edge_decoder")
        out[(len(program), "decode")] = {"pred": g["field"][:, -2:] + O.edge_scalar_to_node_vector(s, g["edge_index"], unit_inv=g["edgeUnitVectorInverse"])}
    return out


# ------------------------------------------------------------------------------------- end to end
def error_triple(y: Tensor, ref: Tensor) -> Tuple[float, float, float]:
    """(mean, 99.9th percentile, max) of |y - ref|."""
    d = (y.detach().cpu().double() - ref.detach().cpu().double()).abs().flatten()
    return d.mean().item(), d.kthvalue(max(int(0.999 * d.numel()), 1)).values.item(), d.max().item()


# ------------------------------------------------------------------------------------- perturbations (of a reference only)
def wrong_boundary_sender(edge_index: Tensor, boundary: Tensor) -> Tuple[Tensor, int]:
    """The edge list in which ONE boundary edge (an edge whose sender another rank owns; `boundary` = their ids, ascending) takes
    the sender of the next boundary edge with another sender.  Returns (edge list, id of that edge); every index stays in range."""
    row = edge_index[0]
    b = boundary.to(row.device)
    diff = torch.nonzero(row[b[:-1]] != row[b[1:]]).flatten()
    assert diff.numel(), "no two boundary edges with different senders"
    i = int(diff[0])
    ei = edge_index.clone()
    ei[0, b[i]] = row[b[i + 1]]
    return ei, int(b[i])


def rows_moved(ref: Tensor, dst_ids: Sequence[Tensor], src_ids: Sequence[Tensor]) -> Tensor:
    """Per rank, the reference rows `src_ids` placed where `dst_ids` are: what a reference looks like that takes the rows a rank
    stores in one order for another order of the same rows (the unsorted coarse edge order for the target-sorted one)."""
    out = ref.clone()
    for d, s in zip(dst_ids, src_ids):
        out[d.to(ref.device)] = ref[s.to(ref.device)]
    return out
