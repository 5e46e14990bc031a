"""Test-only numpy restatement of g4c_body_forces_adjoint (csrc/body_forces.hip) and of gfd.nn.ForceLoss.  Nothing here calls
graphs4cfd_amd; the forward it transposes is tests/forces_ref.py's.

(a) `node_tables`: item_body; the items grouped by their node (own_off, own_item: a stable argsort of `items`); and the in-list — the
    pairs (w, e), e an in-edge of items[w], in the flat order "w, then CSR position e", stably sorted by e (so: ascending e, ties by
    ascending w) and stably grouped by the sender src[e] — in_off, in_item = w, in_g = g[e] in that order.
(b) `stage`: per item, the fp64 algebra of include/g4c.h, one rounding per operation (numpy never contracts), H [W, 4] = (H[u][0],
    H[u][1], H[v][0], H[v][1]) and cp [W], as fp64 values and with the magnitude of the terms they were summed from.
(c) `adjoint32`: the per-node numpy.float32 loop, bit for bit (the s-th entry of every list at once); `adjoint64`: the same in fp64
    from the unrounded H and cp, with a per-element bound on the fp32 loop's distance from it, u = 2⁻²⁴:
        (n_in + n_diag + 3) u Σ|g · H|  +  Σ|g| (u |H| + 16 · 2⁻⁵³ Σ|terms of H|)                       (velocity columns)
        (n_own + 3) u Σ|cp|  +  Σ (u |cp| + 16 · 2⁻⁵³ Σ|terms of cp|)                                    (the pressure column)
    — the roundings along the two walks (n_in list entries and n_diag = n_own · deg diagonal entries), the rounding of H and cp to
    fp32, and the few fp64 roundings of (b) that a cancellation could magnify.
(d) `forward64`: forces_ref.terms and sum_plain with the gradient in fp64 too: the linear map J (and its constant) whose transpose
    (c) claims to be.  WRONG names the deliberate mistakes of `adjoint64` the tests must reject.
(e) `ForceRef`: ForceLoss in fp64, its gradient and the allowances of the device's fp32 value and gradient."""
from typing import Optional

import numpy as np

F32, F64, I32 = np.float32, np.float64, np.int32
U = 2.0 ** -24
FPX, FPY, FVX, FVY, MP, MV = range(6)
WRONG = ("no-diagonal", "swapped-axes", "arm-sign", "scales-exchanged", "shifted-list")


# ------------------------------------------------------------------ (a) tables
def item_edges(items, off):
    """(w [Q], e [Q]): every pair (item, CSR position of an in-edge of its node), ordered by w, then e."""
    items, off = np.asarray(items, np.int64), np.asarray(off, np.int64)
    first = off[items]
    deg = off[items + 1] - first
    w = np.repeat(np.arange(items.size, dtype=np.int64), deg)
    e = first[w] + (np.arange(w.size, dtype=np.int64) - (np.cumsum(deg) - deg)[w])
    return w, e


def _group(keys, n):
    perm = np.argsort(keys, kind="stable")
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(keys, minlength=n), out=off[1:])
    return perm, off


def node_tables(items, body_offsets, n_nodes: int, off=None, src=None, g=None, wrong: Optional[str] = None) -> dict:
    items = np.asarray(items, np.int64)
    bo = np.asarray(body_offsets, np.int64)
    own_item, own_off = _group(items, n_nodes)
    t = dict(item_body=np.repeat(np.arange(bo.size - 1), np.diff(bo)).astype(I32), own_off=own_off.astype(I32),
             own_item=own_item.astype(I32))
    if off is not None:
        w, e = item_edges(items, off)
        order = np.argsort(e, kind="stable")
        w, e = w[order], e[order]
        perm, in_off = _group(np.asarray(src, np.int64)[e], n_nodes)
        if wrong == "shifted-list":          # node j walks the list of node j − 1
            in_off = np.concatenate([[0], in_off[:-1]])
        t.update(in_off=in_off.astype(I32), in_item=w[perm].astype(I32), in_g=np.ascontiguousarray(np.asarray(g, F32)[e[perm]]).reshape(-1, 2))
    return t


# ------------------------------------------------------------------ (b) per item
def stage(gF, gwall, geo, item_body, *, mu=0.0, p_scale=1.0, u_scale=1.0, v_scale=1.0, wrong=None, **_):
    """(H [W, 4] fp64, cp [W] fp64, Σ|terms| of H [W, 4], of cp [W])."""
    n_items = int(np.asarray(item_body).size)
    gf = np.zeros((max(int(np.max(item_body, initial=-1)) + 1, 1), 6), F64) if gF is None else np.asarray(gF, F64)
    gw = np.zeros((n_items, 2), F64) if gwall is None else np.asarray(gwall).astype(F64)
    f = gf[np.asarray(item_body, np.int64)] if n_items else np.zeros((0, 6))
    ax, ay, rx, ry = geo["area"][:, 0], geo["area"][:, 1], geo["arm"][:, 0], geo["arm"][:, 1]
    mu, p_scale, u_scale, v_scale = F64(mu), F64(p_scale), F64(u_scale), F64(v_scale)
    if wrong == "scales-exchanged":
        u_scale, v_scale = v_scale, u_scale
    H, Hm = np.zeros((n_items, 4), F64), np.zeros((n_items, 4), F64)
    if mu != 0:
        gs = gw[:, 1]
        nx, ny = geo["unit"][:, 0], geo["unit"][:, 1]
        tx, ty = -ny, nx
        m0, m1 = ry * f[:, MV], rx * f[:, MV]
        if wrong == "arm-sign":
            m0, m1 = -m0, -m1
        A, Bc = f[:, FVX] - m0, f[:, FVY] + m1
        Am, Bm = np.abs(f[:, FVX]) + np.abs(m0), np.abs(f[:, FVY]) + np.abs(m1)
        sxx, sxy, syy = gs * (tx * nx), gs * (ty * nx + tx * ny), gs * (ty * ny)
        dxx = mu * (A * ax + sxx)
        dxy = mu * ((A * ay + Bc * ax) + sxy)
        dyy = mu * (Bc * ay + syy)
        mxx = np.abs(mu) * (Am * np.abs(ax) + np.abs(sxx))
        mxy = np.abs(mu) * (Am * np.abs(ay) + Bm * np.abs(ax) + np.abs(gs) * (np.abs(ty * nx) + np.abs(tx * ny)))
        myy = np.abs(mu) * (Bm * np.abs(ay) + np.abs(syy))
        H = np.stack([u_scale * (2.0 * dxx), u_scale * dxy, v_scale * dxy, v_scale * (2.0 * dyy)], axis=1)
        Hm = np.stack([np.abs(u_scale) * 2.0 * mxx, np.abs(u_scale) * mxy, np.abs(v_scale) * mxy, np.abs(v_scale) * 2.0 * myy], axis=1)
        if wrong == "swapped-axes":
            H = H[:, [1, 0, 3, 2]]
    fa, fb = f[:, FPX] * ax, f[:, FPY] * ay
    c0, c1 = rx * ay, ry * ax
    mp = f[:, MP] * (c0 - c1)
    cp = p_scale * (gw[:, 0] - ((fa + fb) + mp))
    cpm = np.abs(p_scale) * (np.abs(gw[:, 0]) + np.abs(fa) + np.abs(fb) + np.abs(f[:, MP]) * (np.abs(c0) + np.abs(c1)))
    return H, cp, Hm, cpm


# ------------------------------------------------------------------ (c) per node
def _walk(H, cp, t, n_nodes, nf, dtype, *, pcol, ucol=0, vcol=1, mu=0.0, off=None, g=None, wrong=None, eH=None, ecp=None, **_):
    """(gx [N, nf] in `dtype`, Σ|products| [N, nf], entries walked [N, nf], Σ|g| eH + Σ ecp [N, nf])."""
    H, cp = np.asarray(H).astype(dtype), np.asarray(cp).astype(dtype)
    eH = np.zeros(H.shape) if eH is None else eH
    ecp = np.zeros(cp.shape) if ecp is None else ecp
    gx, mag, cnt, err = (np.zeros((n_nodes, nf), d) for d in (dtype, F64, np.int64, F64))
    own_off, own_item = t["own_off"].astype(np.int64), t["own_item"].astype(np.int64)
    n_own = np.diff(own_off)
    p, pm, pe = np.zeros(n_nodes, dtype), np.zeros(n_nodes), np.zeros(n_nodes)
    for s in range(int(n_own.max()) if n_nodes and n_own.size else 0):
        nodes = np.nonzero(n_own > s)[0]
        w = own_item[own_off[nodes] + s]
        p[nodes] = (p[nodes] + cp[w]).astype(dtype)
        pm[nodes] += np.abs(cp[w].astype(F64))
        pe[nodes] += ecp[w]
    gx[:, pcol], mag[:, pcol], cnt[:, pcol], err[:, pcol] = p, pm, n_own, pe
    if mu != 0:
        g = np.asarray(g).astype(dtype)
        in_g = t["in_g"].astype(dtype)
        in_off, in_item, off = t["in_off"].astype(np.int64), t["in_item"].astype(np.int64), np.asarray(off, np.int64)
        acc, am, ae = np.zeros((n_nodes, 2), dtype), np.zeros((n_nodes, 2)), np.zeros((n_nodes, 2))

        def add(nodes, ge, w, sign):
            for a in (0, 1):
                for f in (0, 1):
                    pr = (ge[:, a] * H[w, 2 * f + a]).astype(dtype)
                    acc[nodes, f] = (acc[nodes, f] + pr).astype(dtype) if sign > 0 else (acc[nodes, f] - pr).astype(dtype)
                    am[nodes, f] += np.abs(pr.astype(F64))
                    ae[nodes, f] += np.abs(ge[:, a].astype(F64)) * eH[w, 2 * f + a]

        n_in = np.diff(in_off)
        for s in range(int(n_in.max()) if n_in.size else 0):
            nodes = np.nonzero(n_in > s)[0]
            q = in_off[nodes] + s
            add(nodes, in_g[q], in_item[q], +1)
        deg = np.diff(off)
        if wrong != "no-diagonal":
            for k in range(int(n_own.max()) if n_own.size else 0):
                mine = np.nonzero(n_own > k)[0]
                for s in range(int(deg[mine].max()) if mine.size else 0):
                    nodes = mine[deg[mine] > s]
                    add(nodes, g[off[nodes] + s], own_item[own_off[nodes] + k], -1)
        for f, c in ((0, ucol), (1, vcol)):
            gx[:, c], mag[:, c], cnt[:, c], err[:, c] = acc[:, f], am[:, f], n_in + n_own * deg, ae[:, f]
    return gx, mag, cnt, err


def adjoint32(gF, gwall, geo, t, n_nodes, nf, **c) -> np.ndarray:
    """gx float32 [N, nf]: the contract's two loops, H and cp rounded to fp32 once."""
    H, cp, _, _ = stage(gF, gwall, geo, t["item_body"], **c)
    return _walk(H.astype(F32), cp.astype(F32), t, n_nodes, nf, F32, **c)[0]


def adjoint64(gF, gwall, geo, t, n_nodes, nf, wrong=None, **c):
    """(gx in fp64 from the unrounded H and cp, the bound of the module docstring)."""
    H, cp, Hm, cpm = stage(gF, gwall, geo, t["item_body"], wrong=wrong, **c)
    eH, ecp = U * np.abs(H) + 16 * 2.0 ** -53 * Hm, U * np.abs(cp) + 16 * 2.0 ** -53 * cpm
    gx, mag, cnt, err = _walk(H, cp, t, n_nodes, nf, F64, wrong=wrong, eH=eH, ecp=ecp, **c)
    return gx, (cnt + 3) * U * mag + err


def abs_adjoint(eF, ewall, geo, t, n_nodes, nf, **c) -> np.ndarray:
    """|Jᵀ| (eF, ewall) for errors eF, ewall >= 0: how far an error in the incoming gradients reaches (every term taken positive)."""
    ageo = dict(area=np.abs(geo["area"]), arm=np.abs(geo["arm"]), unit=np.abs(geo["unit"]))
    _, _, Hm, cpm = stage(np.abs(eF) if eF is not None else None, np.abs(ewall) if ewall is not None else None, ageo, t["item_body"], **c)
    ta = dict(t)
    if "in_g" in t:
        ta["in_g"] = np.abs(t["in_g"])
    cc = dict(c)
    g = cc.pop("g", None)
    gx = _walk(Hm, cpm, ta, n_nodes, nf, F64, g=None if g is None else np.abs(g), **cc)
    # (the diagonal is subtracted by the walk: its magnitude is what counts)
    return gx[1]


# ------------------------------------------------------------------ (d) the forward in fp64
def forward64(x, geo, *, pcol, ucol=0, vcol=1, mu=0.0, p_scale=1.0, p_shift=0.0, u_scale=1.0, v_scale=1.0, off=None, g=None, src=None, **_):
    """(S [B, 6], wall [W, 2], G [W, 4], Σ|g · diff| [W, 4]) of the fp64 fields x: forces_ref.terms with an fp64 gradient, plain sums."""
    x = np.asarray(x, F64)
    it = np.asarray(geo["items"], np.int64)
    n_items = it.size
    ax, ay, rx, ry = geo["area"][:, 0], geo["area"][:, 1], geo["arm"][:, 0], geo["arm"][:, 1]
    P = F64(p_scale) * x[it, pcol] + F64(p_shift)
    T = np.zeros((n_items, 6))
    T[:, FPX], T[:, FPY] = -(P * ax), -(P * ay)
    T[:, MP] = rx * T[:, FPY] - ry * T[:, FPX]
    G, Gm, shear = np.zeros((n_items, 4)), np.zeros((n_items, 4)), np.zeros(n_items)
    if mu != 0:
        w, e = item_edges(it, off)
        s = np.asarray(src, np.int64)[e]
        g64 = np.asarray(g, F32).astype(F64)
        for f, col in ((0, ucol), (1, vcol)):
            diff = x[s, col] - x[it[w], col]
            for a in (0, 1):
                np.add.at(G[:, 2 * f + a], w, g64[e, a] * diff)
                np.add.at(Gm[:, 2 * f + a], w, np.abs(g64[e, a] * diff))
        ugx, ugy, vgx, vgy = F64(u_scale) * G[:, 0], F64(u_scale) * G[:, 1], F64(v_scale) * G[:, 2], F64(v_scale) * G[:, 3]
        sxx, sxy, syy = 2.0 * ugx, ugy + vgx, 2.0 * vgy
        T[:, FVX], T[:, FVY] = F64(mu) * (sxx * ax + sxy * ay), F64(mu) * (sxy * ax + syy * ay)
        T[:, MV] = rx * T[:, FVY] - ry * T[:, FVX]
        nx, ny = geo["unit"][:, 0], geo["unit"][:, 1]
        tx, ty = -ny, nx
        shear = F64(mu) * ((tx * sxx + ty * sxy) * nx + (tx * sxy + ty * syy) * ny)
    bo = np.asarray(geo["body_offsets"], np.int64)
    S = np.stack([T[a:b].sum(0) for a, b in zip(bo[:-1], bo[1:])]) if bo.size > 1 else np.zeros((0, 6))
    return S, np.stack([P, shear], axis=1), G, Gm


def inner(S, wall, gF, gwall) -> float:
    return float((S * (0 if gF is None else np.asarray(gF, F64))).sum() + (wall * (0 if gwall is None else np.asarray(gwall, F64))).sum())


# ------------------------------------------------------------------ (e) ForceLoss in fp64
COMPONENTS = {"fx": (FPX, FVX), "fy": (FPY, FVY), "m": (MP, MV)}


class ForceRef:
    """gfd.nn.ForceLoss in fp64 on the device's own tables: node_weight · GraphLoss + weight · mean_{b, c} ((F_c(pred) − F_ref)/force_scale)²
    + wp · mean_w ΔP² + ws · mean_w Δshear²; `consts` the keywords of forward64 / adjoint64 (columns, constants, off, g, src)."""

    def __init__(self, geo, n_nodes, consts, weight=1.0, node_weight=1.0, lambda_d=0.0, dirichlet=None, components=("fx", "fy"),
                 force_scale=1.0, wall=None):
        self.geo, self.n, self.c = geo, n_nodes, consts
        self.weight, self.node_weight, self.lambda_d, self.dirichlet = weight, node_weight, lambda_d, dirichlet
        self.components, self.force_scale = tuple(components), force_scale
        self.wp, self.ws = (0.0, 0.0) if wall is None else (wall.get("pressure", 0.0), wall.get("shear", 0.0))
        self.tables = node_tables(geo["items"], geo["body_offsets"], n_nodes, consts.get("off"), consts.get("src"), consts.get("g"))

    def _base64(self, p, t):
        d = p - t
        val = float((d * d).mean())
        if self.lambda_d > 0 and self.dirichlet is not None and self.dirichlet.any():
            val += self.lambda_d * float(np.abs(d[self.dirichlet]).mean())
        return val

    def _total(self, S):
        return np.stack([S[:, COMPONENTS[c][0]] + S[:, COMPONENTS[c][1]] for c in self.components], axis=1)

    def _parts(self, p, t, values):
        """(ΔF / force_scale [B, C], Δwall [W, 2], Σ|g diff| of pred's gradient)."""
        Sp, wp, _, Gm = forward64(p, self.geo, **self.c)
        St, wt, _, Gt = forward64(t, self.geo, **self.c)
        ref = self._total(St) if values is None else np.asarray(values, F64)
        return (self._total(Sp) - ref) / self.force_scale, wp - wt, Gm, Gt

    def loss(self, pred, target, values=None) -> float:
        """The value in fp64 from fp64 inputs (a difference quotient of it means something)."""
        p, t = np.asarray(pred, F64), np.asarray(target, F64)
        val = self.node_weight * self._base64(p, t) if self.node_weight > 0 else 0.0
        dF, dW, _, _ = self._parts(p, t, values)
        if self.weight > 0:
            val += self.weight * float((dF * dF).mean())
        if self.wp > 0:
            val += self.wp * float((dW[:, 0] ** 2).mean())
        if self.ws > 0:
            val += self.ws * float((dW[:, 1] ** 2).mean())
        return val

    def _incoming(self, dF, dW):
        """(gF [B, 6], gwall [W, 2]) of the loss in fp64."""
        gF = np.zeros((dF.shape[0], 6))
        if self.weight > 0:
            y = 2.0 * self.weight * dF / (dF.size * self.force_scale)
            for k, c in enumerate(self.components):
                for col in COMPONENTS[c]:
                    gF[:, col] += y[:, k]
        gw = np.stack([2.0 * self.wp * dW[:, 0] / max(dW.shape[0], 1), 2.0 * self.ws * dW[:, 1] / max(dW.shape[0], 1)], axis=1)
        return gF, gw

    def _forward_errors(self, p, t, Gm, Gt, measured=False):
        """How far the device's (ΔF / force_scale, Δwall) may sit from the fp64 ones: the fp32 gradient loops at the wall nodes —
        (deg + 3) u Σ|g · diff| per accumulator, forces_ref.gradient_bound's second term, for pred and for target — carried through
        the (linear, fp64) stress algebra with every coefficient taken positive, the fp64 sums' own roundings (forces_ref.sum_bound's
        2 (n + 4) 2⁻⁵³ Σ|terms| is below 1e-6 of that and folded into the factor), and the (float) casts of wall: u |wall| each."""
        c = self.c
        it = np.asarray(self.geo["items"], np.int64)
        deg = np.diff(np.asarray(c["off"], np.int64))[it] if c.get("mu", 0.0) != 0 else np.zeros(it.size)
        if measured:          # F_ref is given: only the wall term launches on the target
            eF = self._forward_errors(p, t, Gm, 0 * Gt)[0]
            return eF, self._forward_errors(p, t, Gm, Gt)[1]
        eG = (deg[:, None] + 3) * U * (Gm + Gt) * (1 + 1e-3)
        ageo = dict(self.geo, area=np.abs(self.geo["area"]), arm=np.abs(self.geo["arm"]), unit=np.abs(self.geo["unit"]))
        mu, us, vs = abs(c.get("mu", 0.0)), abs(c.get("u_scale", 1.0)), abs(c.get("v_scale", 1.0))
        ax, ay, rx, ry = ageo["area"][:, 0], ageo["area"][:, 1], ageo["arm"][:, 0], ageo["arm"][:, 1]
        sxx, sxy, syy = 2 * us * eG[:, 0], us * eG[:, 1] + vs * eG[:, 2], 2 * vs * eG[:, 3]
        T = np.zeros((it.size, 6))
        T[:, FVX], T[:, FVY] = mu * (sxx * ax + sxy * ay), mu * (sxy * ax + syy * ay)
        T[:, MV] = rx * T[:, FVY] + ry * T[:, FVX]
        nx, ny = ageo["unit"][:, 0], ageo["unit"][:, 1]
        esh = mu * ((ny * sxx + nx * sxy) * nx + (ny * sxy + nx * syy) * ny)
        bo = np.asarray(self.geo["body_offsets"], np.int64)
        eS = np.stack([T[a:b].sum(0) for a, b in zip(bo[:-1], bo[1:])])
        _, wp, _, _ = forward64(p, self.geo, **c)
        _, wt, _, _ = forward64(t, self.geo, **c)
        eW = np.stack([np.zeros(it.size), esh], axis=1) + U * (np.abs(wp) + np.abs(wt)) + U * np.abs(wp - wt)
        return self._total(eS) / self.force_scale * (1 + 1e-6), eW

    def value(self, pred, target, values=None):
        """(the loss in fp64 from the fp32 inputs, how far the device's value may sit from it): GraphLoss's fp32 mean as in
        sample_adjoint_ref.SampleRef.value ((M + 6) u of it), the force term — fp64 on the device until its mean, then one cast —
        carries the forward's error into its squares, 2 |d| e + e², and the wall terms the same plus an fp32 mean of W terms."""
        p, t = np.asarray(pred, F32).astype(F64), np.asarray(target, F32).astype(F64)
        val = self.loss(p, t, values)
        base = self.node_weight * self._base64(p, t) if self.node_weight > 0 else 0.0
        dF, dW, Gm, Gt = self._parts(p, t, values)
        eF, eW = self._forward_errors(p, t, Gm, Gt, measured=values is not None)
        allowed = (p.size + 6) * U * base + 6 * U * val
        if self.weight > 0:
            allowed += self.weight * float((2 * np.abs(dF) * eF + eF * eF).mean())
        for wgt, k in ((self.wp, 0), (self.ws, 1)):
            if wgt > 0:
                allowed += wgt * float((2 * np.abs(dW[:, k]) * eW[:, k] + eW[:, k] ** 2).mean()) + (dW.shape[0] + 6) * U * wgt * float((dW[:, k] ** 2).mean())
        return val, allowed

    def grad(self, pred, target, values=None):
        """(∂loss/∂pred in fp64 from the fp32 inputs, how far the device's fp32 gradient may sit from it): GraphLoss's own gradient (7 u of
        its magnitude) and autograd's sums of the parts (one rounding per addition: 4 u of the magnitudes added); the incoming (gF,
        gwall) carry the forward's error times their scale plus five roundings of their own; Jᵀ of that error by `abs_adjoint`, and
        the adjoint's own bound (`adjoint64`).  The force and the wall gradients arrive in separate backward launches and are added
        in fp32."""
        import adjoint_op_ref as A
        p, t = np.asarray(pred, F32).astype(F64), np.asarray(target, F32).astype(F64)
        n, nf = p.shape
        total, allowed, size = np.zeros((n, nf)), np.zeros((n, nf)), np.zeros((n, nf))
        if self.node_weight > 0:
            base = A.graph_loss64(pred, target, self.lambda_d, self.dirichlet)[1]
            mse = A.graph_loss64(pred, target, 0.0, None)[1]
            size = self.node_weight * (np.abs(mse) + np.abs(base - mse))
            total, allowed = self.node_weight * base, 7 * U * size
        dF, dW, Gm, Gt = self._parts(p, t, values)
        eF, eW = self._forward_errors(p, t, Gm, Gt, measured=values is not None)
        gF, gw = self._incoming(dF, dW)
        c = {k: v for k, v in self.c.items() if k not in ("p_shift", "src")}
        egF = np.zeros_like(gF)
        if self.weight > 0:
            ey = 2.0 * self.weight * eF / (dF.size * self.force_scale)
            for k, cname in enumerate(self.components):
                for col in COMPONENTS[cname]:
                    egF[:, col] += ey[:, k]
        egF += 5 * U * np.abs(gF)
        egw = np.stack([2.0 * self.wp * eW[:, 0], 2.0 * self.ws * eW[:, 1]], axis=1) / max(dW.shape[0], 1) + 5 * U * np.abs(gw)
        parts = []
        if self.weight > 0:
            parts.append((gF, None, egF, None))
        if self.wp > 0 or self.ws > 0:
            parts.append((None, gw, None, egw))
        for a, b, ea, eb in parts:
            gx, bound = adjoint64(a, b, self.geo, self.tables, n, nf, **c)
            if b is not None:          # (gwall reaches the launch as fp32: its cast is one rounding more)
                eb = eb + U * np.abs(b)
            reach = abs_adjoint(ea, eb, self.geo, self.tables, n, nf, **c)
            total = total + gx
            size = size + np.abs(gx)
            allowed = allowed + (bound + reach) * (1 + 1e-3)
        return total, allowed + 4 * U * size


# ------------------------------------------------------------------ the synthetic inputs of the GPU tests
LIST_LENGTHS = (0, 1, 3, 4, 5, 9)          # around the unroll of four
HUB = 300                                  # wall items fed by one sender: more than a workgroup has threads


def synthetic(n_nodes: int, n_items: int, n_bodies: int, seed: int = 0, max_deg: int = 6):
    """(geo, off, src, g) of no mesh and no polygon — the launch trusts its tables, the restatement needs only items, off, g, src:
    node k < 6 is an item LIST_LENGTHS[k] times (its own-list) and node 6 + k sends exactly LIST_LENGTHS[k] edges to wall nodes (its
    in-list); node 12 is in no table at all; node 13 sends one edge to each of HUB wall nodes; node 14 is a wall node whose weights
    are zero (degenerate); every other item is a random node from 16 on, every other sender a random node from 16 on.  Random fp64
    geometry with unit normals; bodies of random sizes."""
    rng = np.random.default_rng(1000 * n_nodes + n_items + seed)
    head = np.repeat(np.arange(6), LIST_LENGTHS)
    once = rng.permutation(np.arange(16, n_nodes))[:n_items - head.size - 1]          # the items that are an item once
    assert once.size == n_items - head.size - 1 and once.size >= HUB + sum(LIST_LENGTHS)
    items = np.concatenate([head, [14], once])
    order = rng.permutation(n_items)
    items = items[order]
    cuts = np.sort(rng.permutation(np.arange(1, n_items))[:n_bodies - 1])
    body_offsets = np.concatenate([[0], cuts, [n_items]]).astype(I32)
    deg = rng.integers(0, max_deg + 1, n_nodes)
    deg[once[:HUB + sum(LIST_LENGTHS)]] = np.maximum(deg[once[:HUB + sum(LIST_LENGTHS)]], 1)
    deg[12] = 0
    deg[14] = 5
    off = np.zeros(n_nodes + 1, np.int64)
    np.cumsum(deg, out=off[1:])
    src = rng.integers(16, n_nodes, int(off[-1]))
    g = rng.standard_normal((int(off[-1]), 2)).astype(F32)
    g[off[14]:off[15]] = 0.0
    # plant the controlled senders on the first in-edge of nodes that are an item once
    plant = once[:HUB + sum(LIST_LENGTHS)]
    src[off[plant[:HUB]]] = 13
    at = HUB
    for k, m in enumerate(LIST_LENGTHS):
        src[off[plant[at:at + m]]] = 6 + k
        at += m
    area, arm = rng.standard_normal((n_items, 2)), rng.standard_normal((n_items, 2))
    unit = rng.standard_normal((n_items, 2))
    unit /= np.sqrt((unit * unit).sum(1))[:, None]
    geo = dict(items=items, body_offsets=body_offsets, area=area, unit=unit, arm=arm, n_bodies=n_bodies)
    return geo, off.astype(I32), src.astype(I32), g


def incoming(n_bodies: int, n_items: int, seed: int = 0):
    rng = np.random.default_rng(77 * n_bodies + n_items + seed)
    return rng.standard_normal((n_bodies, 6)), rng.standard_normal((n_items, 2)).astype(F32)


BIG = 270_000          # > 262 144 = 1024 workgroups of 256 nodes: the grid-stride loop takes a second pass
