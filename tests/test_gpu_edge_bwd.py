"""EdgeConv's backward kernel by kernel through the C ABI: pf_edge_backward_sums_f32 (edge_bwd_reduce_kernel<32|64, 16|0>),
pf_edge_backward_coeffs_f32 and pf_edge_backward_finish_f32 (edge_bwd_inverse_kernel<32|64>), each against a float64
evaluation of the closed form stated above EdgeBwdAffine in csrc/edgeconv.hip, given the previous stage's ACTUAL output, and
the three composed against the closed form run end to end.  No convolution runs: [l | e] rows, the upstream gradient (in a
wider buffer, ldg > cbn, NaN in the columns no kernel may read), the four affine rows (float64 statistics of the data with
gamma / beta / eps, rounded to float32: what the finalize launch hands over) and idx are built here; idx by a builder that
PRESCRIBES in-degrees, so that the inverted lists sit on the boundaries of the finish pass's walk (its own Q-wide chunks,
HEAD = 24, the shared hub tail's trips of 4 NG pairs, a second trip, lists of ~1000 and 5000) with hubs in the first and
last row group of a wave, two in one wave, in the last block among lanes without a row, and in a wave that straddles two
groups (the tail's `!same` arm).

The ReLU mask needs no tolerance and no excluded point.  Both passes compute d = e - l as ONE float32 subtraction and
u = fmaf(d, a, b); the reference takes d as the float32 difference (torch's float32 subtraction: the same bits) and decides
u > 0 as double(d) * double(a) + double(b) > 0.  The product of two float32 numbers is exact in float64 and rounding a sum
never moves it across zero, so that sign is fmaf's.  A result that disagrees is not a mask flip.

Gates are counted, never picked: |got - ref| <= K * 2^-24 * A, A = the reference expression with every product and term
replaced by its absolute value, K = twice the float32 roundings on the kernel's path (the R_* counts below, next to the
expression they count).  Sums the kernel carries in float64 get the roundings of their float32 terms plus 2 n 2^-53 A for
the n float64 additions of either side.  Every test reports its worst |got - ref| / gate per quantity.  Every call is made
twice and must give the same bits.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, report
from pointmvsnet_amd import _lib, pointflow

gpu = pytest.mark.gpu

U = 2.0 ** -24                       # unit roundoff of float32
U64 = 2.0 ** -53
F32, F64 = torch.float32, torch.float64
EPS = 1e-5
TILE = 64                            # PF_GEMM_TILE: points per tile of the stats / apply / reduce passes


def _kernel_constants():
    """HEAD and the finish pass's block cap as csrc/edgeconv.hip spells them (the list lengths below sit on them)"""
    with open(os.path.join(ROOT, "pointmvsnet_amd", "csrc", "edgeconv.hip")) as f:
        src = f.read()
    head = re.findall(r"constexpr uint32_t HEAD = (\d+);", src)
    cap = re.findall(r"if \(blocks > (\d+)\) blocks = (\d+);", src)
    assert len(head) == 1 and len(cap) == 1 and cap[0][0] == cap[0][1]
    return int(head[0]), int(cap[0][0])


HEAD, FINISH_CAP = _kernel_constants()

# float32 roundings on the kernel's path, per value (edgeconv.hip, edge_bwd_reduce_kernel / edge_bwd_inverse_kernel;
# -ffp-contract=off: the arithmetic is as written; 0 + x is exact, so n terms cost n - 1 additions)
R_SG = lambda k: 1 + (k - 1)             # gd = gy / kf; sg += gg                                            # noqa: E731
R_SGX = lambda k: 4 + (k - 1)            # gd; d - mv; * iv; gg * .; sx += .                                   # noqa: E731
R_SX = lambda k: (k - 1) + 3             # sd += d; kf * mv; sd - .; * iv                                      # noqa: E731
R_CENTRAL_GX = 3                         # l - mc; * ic; gg * .   (sum g_c itself: float32 inputs added in float64, 0)
R_CAST = 1                               # (float)(float64 sum / m), (float)sum
R_DL = 5                                 # kf * c1; sg - .; c2 * sx; . - .; av * .
R_DL_CONCAT = 7                          # central term: gg - c1c; l - mc; * ic; * c2c; . - .; ac * .; then dl += .
R_PAIR = 7                               # gy / kf; gg - c1; d - mv; * iv; * c2; . - .; av * .
R_DE = lambda length: R_PAIR + length    # + one addition per pair of the list, however the wave shares them  # noqa: E731


# ---------------------------------------------------------------------------------------------
# index lists with prescribed in-degrees
# ---------------------------------------------------------------------------------------------
def build_idx(Ng, k, wanted, empty, seed):
    """idx (Ng, k) int64, group-local targets: row r is named exactly wanted[r] times, the rows of `empty` never, what is
    left of the Ng * k pairs is dealt evenly to the other rows; pair positions are a seeded permutation."""
    assert not (set(wanted) & set(empty))
    ordinary = np.array([r for r in range(Ng) if r not in wanted and r not in empty], dtype=np.int64)
    left = Ng * k - sum(wanted.values())
    assert left >= 0 and (left == 0 or len(ordinary) > 0)
    targets = [np.full(n, r, dtype=np.int64) for r, n in sorted(wanted.items())]
    if left:
        targets.append(np.resize(ordinary, left))
    targets = np.concatenate(targets)
    assert targets.size == Ng * k
    rng = np.random.RandomState(seed)
    idx = torch.from_numpy(targets[rng.permutation(targets.size)].reshape(Ng, k).copy())
    deg = torch.bincount(idx.reshape(-1), minlength=Ng)
    for r, n in wanted.items():
        assert int(deg[r]) == n, (r, n, int(deg[r]))
    for r in empty:
        assert int(deg[r]) == 0
    assert int((deg == 0).sum()) >= 1                                  # a condition of the test, not something to tolerate
    return idx


def hub_lengths(C, k):
    """the list lengths of the issue for C (Q lanes per row, NG row groups per wave); the reduced set for k != 16"""
    Q, NG = C // 4, 64 // (C // 4)
    if k == 16:
        return [0, 1, Q - 1, Q, Q + 1, HEAD - 1, HEAD, HEAD + 1, HEAD + NG - 1, HEAD + NG, HEAD + NG + 1,
                HEAD + 4 * NG - 1, HEAD + 4 * NG, HEAD + 4 * NG + 1, HEAD + 8 * NG + 3, 1003, 5001]
    if k == 5:
        return [0, 1, Q + 1, HEAD, HEAD + 1, HEAD + NG + 1, HEAD + 4 * NG + 1, HEAD + 8 * NG + 3, 1003]
    return [0, 1, HEAD, HEAD + 1, HEAD + 4 * NG + 1, HEAD + 8 * NG + 3]


def hub_layout(C, k, G, Ng):
    """per group {local row: length} and the never-gathered rows.  Placements (rows are global = g * Ng + local; a wave
    holds NG consecutive rows, a block 256 / Q):  the two longest lists in the first and the last row group of one wave (two
    hubs in one wave); the third longest on the very last row (its block has lanes without a row: G * Ng is no multiple of
    256 / Q); with G > 1 two lists beyond HEAD on the last row of group 0 and the first of group 1, which share a wave
    because Ng is no multiple of NG (the `!same` arm); the rest on rows 2 waves apart, alternating first / last row group."""
    Q = C // 4
    NG, PPB = 64 // Q, 256 // Q
    assert (G * Ng) % PPB != 0 and (G == 1 or Ng % NG != 0)
    lengths = sorted(hub_lengths(C, k), reverse=True)
    out = []
    for g in range(G):
        base = g * Ng
        first_wave = -(-base // NG) + 2                                  # a wave that lies wholly inside the group
        taken, wanted, empty = set(), {}, []

        def put(local, n):
            assert 0 <= local < Ng and local not in taken
            taken.add(local)
            if n == 0:
                empty.append(local)
            else:
                wanted[local] = n

        rest = list(lengths)
        w0 = first_wave * NG - base
        put(w0, rest.pop(0))                                             # first row group of a wave ...
        put(w0 + NG - 1, rest.pop(0))                                    # ... and the last of the SAME wave
        if g == G - 1:
            put(Ng - 1, rest.pop(0))                                     # the last row of the launch
        if G > 1 and g == 0:
            put(Ng - 1, HEAD + 4 * NG + 2)                               # straddling wave, owner in group 0 (two trips alone)
        if G > 1 and g == 1:
            put(0, HEAD + 2)                                             # the same wave, owner in group 1
        for i, n in enumerate(rest):
            wave = first_wave + 2 + 2 * i
            put(wave * NG - base + (0 if i % 2 == 0 else NG - 1), n)
        out.append((wanted, empty))
    return out


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
class Case(object):
    pass


def make_case(C, k, G, Ng, gps, concat, idx, seed, dtype=F32, ldg_extra=8, ld_extra=0):
    """LE (G * Ng, 2C), the upstream gradient inside a (G * Ng, cbn + ldg_extra) buffer, the affine rows (S, cbn +
    ld_extra): float64 statistics of the data per statistic set, gamma, beta, eps, rounded to `dtype`."""
    c = Case()
    c.C, c.k, c.G, c.Ng, c.gps, c.concat = C, k, G, Ng, gps, int(bool(concat))
    c.R, c.S, c.cbn, c.doff = G * Ng, G // gps, (2 * C if concat else C), (C if concat else 0)
    c.ldg, c.ld = c.cbn + ldg_extra, c.cbn + ld_extra
    gen = torch.Generator().manual_seed(seed)
    c.LE = (torch.randn(c.R, 2 * C, generator=gen, dtype=F64) * 0.8 + 0.1).to(dtype)
    c.gy_buf = torch.full((c.R, c.ldg), float("nan"), dtype=dtype)
    c.gy_buf[:, :c.cbn] = torch.randn(c.R, c.cbn, generator=gen, dtype=F64).to(dtype)
    c.gy = c.gy_buf[:, :c.cbn]
    c.idx = idx.reshape(G, Ng, k).contiguous()
    c.nb = c.idx.clamp(0, Ng - 1) + torch.arange(G).view(G, 1, 1) * Ng          # the forward's clamp, global rows
    c.gamma = 1.0 + 0.4 * torch.randn(c.cbn, generator=gen, dtype=F64)
    c.gamma[::5] *= -1.0
    c.beta = 0.3 * torch.randn(c.cbn, generator=gen, dtype=F64)
    rows = torch.zeros(4, c.S, c.ld, dtype=F64)
    for s in range(c.S):
        r0, r1 = s * gps * Ng, (s + 1) * gps * Ng
        l = c.LE[r0:r1, :C]
        d = (c.LE[:, C:][c.nb.reshape(c.R, k)[r0:r1]] - l[:, None, :]).double().reshape(-1, C)
        x = torch.cat([l.double().repeat_interleave(k, 0), d], 1) if concat else d
        mean, var = x.mean(0), x.var(0, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + EPS)
        rows[0, s, :c.cbn] = c.gamma * invstd
        rows[1, s, :c.cbn] = c.beta - mean * c.gamma * invstd
        rows[2, s, :c.cbn] = mean
        rows[3, s, :c.cbn] = invstd
    c.scale, c.shift, c.mean, c.invstd = [r.to(dtype).contiguous() for r in rows]
    return c


@functools.lru_cache(maxsize=None)
def hub_case(C, k, G, gps, concat):
    Ng = {16: 1037, 5: 1203, 1: 1101}[k]
    idx = torch.stack([build_idx(Ng, k, w, e, 100 * g + C + k) for g, (w, e) in enumerate(hub_layout(C, k, G, Ng))])
    return make_case(C, k, G, Ng, gps, concat, idx, seed=C + 7 * k + G + gps + concat,
                     ld_extra=4 if (G > 1 and gps == 1) else 0)


# ---------------------------------------------------------------------------------------------
# the closed form in float64 (edgeconv.hip, above EdgeBwdAffine), stage by stage
# ---------------------------------------------------------------------------------------------
def _aff(c, g, off):
    s = g // c.gps
    return [r[s, off:off + c.C].double() for r in (c.scale, c.shift, c.mean, c.invstd)]


def _group(c, g):
    """d, g_j = [u_j > 0] G / k, xhat_j and |xhat|'s majorant for the pairs of group g: (Ng, k, C) float64 each"""
    C, r0 = c.C, g * c.Ng
    l = c.LE[r0:r0 + c.Ng, :C]
    d = (c.LE[:, C:][c.nb[g]] - l[:, None, :]).double()       # ONE subtraction in LE's dtype: the kernel's float32 d
    a, b, mu, istd = _aff(c, g, c.doff)
    mask = (d * a + b) > 0                                      # exact product, one rounding: the sign of fmaf(d, a, b)
    gj = mask * (c.gy[r0:r0 + c.Ng, c.doff:c.doff + C].double() / c.k)[:, None, :]
    return d, gj, (d - mu) * istd, (d.abs() + mu.abs()) * istd, a


def _central(c, g):
    """g_c = [u_c > 0] G_c, xhat_c and its majorant: (Ng, C)"""
    C, r0 = c.C, g * c.Ng
    l = c.LE[r0:r0 + c.Ng, :C].double()
    a, b, mu, istd = _aff(c, g, 0)
    gc = ((l * a + b) > 0) * c.gy[r0:r0 + c.Ng, :C].double()
    return gc, (l - mu) * istd, (l.abs() + mu.abs()) * istd, a


def ref_sums(c):
    """P (G, cbn, 2) = per group (sum g, sum g * xhat) per BatchNorm column, the rows [sum_j g_j | sum_j xhat_j], the
    majorants A of each and the gates."""
    C, k, o = c.C, c.k, Case()
    o.P, o.PA, o.PK = [torch.zeros(c.G, c.cbn, 2, dtype=F64) for _ in range(3)]
    o.SG, o.SGA, o.SX, o.SXA = [torch.zeros(c.R, C, dtype=F64) for _ in range(4)]
    for g in range(c.G):
        r = slice(g * c.Ng, (g + 1) * c.Ng)
        d, gj, xh, xa, _ = _group(c, g)
        o.SG[r], o.SGA[r], o.SX[r], o.SXA[r] = gj.sum(1), gj.abs().sum(1), xh.sum(1), xa.sum(1)
        o.P[g, c.doff:, 0], o.PA[g, c.doff:, 0] = gj.sum((0, 1)), gj.abs().sum((0, 1))
        o.P[g, c.doff:, 1], o.PA[g, c.doff:, 1] = (gj * xh).sum((0, 1)), (gj.abs() * xa).sum((0, 1))
        o.PK[g, c.doff:, 0], o.PK[g, c.doff:, 1] = R_SG(k), R_SGX(k)
        if c.concat:
            gc, xc, xca, _ = _central(c, g)
            o.P[g, :C, 0], o.PA[g, :C, 0] = gc.sum(0), gc.abs().sum(0)
            o.P[g, :C, 1], o.PA[g, :C, 1] = (gc * xc).sum(0), (gc.abs() * xca).sum(0)
            o.PK[g, :C, 0], o.PK[g, :C, 1] = 0, R_CENTRAL_GX
    # float64 accumulation: at most Ng * k additions on either side
    o.P_gate = (2 * o.PK * U + 2 * c.Ng * k * U64) * o.PA
    o.SG_gate = 2 * R_SG(k) * U * o.SGA
    o.SX_gate = 2 * R_SX(k) * U * o.SXA
    return o


def ref_coeffs(c, P):
    """c1, c2 (S, cbn), dgamma, dbeta (cbn,) from per-group sums P (G, cbn, 2) float64"""
    m = torch.full((c.cbn,), float(c.gps * c.Ng * c.k), dtype=F64)
    if c.concat:
        m[:c.C] = float(c.gps * c.Ng)
    sets = P.reshape(c.S, c.gps, c.cbn, 2).sum(1)
    return sets[..., 0] / m, sets[..., 1] / m, sets[..., 1].sum(0), sets[..., 0].sum(0), m


def ref_finish(c, SG, SX, c1, c2, dSG=None, dSX=None, dc1=None, dc2=None):
    """dl, de (R, C) from the rows [sum g | sum xhat] and c1, c2 (S, cbn), all float64; their majorants; the length of
    every row's list; and, given bounds on the errors of the four inputs, what those add to dl and de (first order)."""
    C, k, o = c.C, c.k, Case()
    o.dl, o.dlA, o.de, o.deA, o.dl_in, o.de_in = [torch.zeros(c.R, C, dtype=F64) for _ in range(6)]
    o.length = torch.bincount(c.nb.reshape(-1), minlength=c.R)
    for g in range(c.G):
        r, s = slice(g * c.Ng, (g + 1) * c.Ng), g // c.gps
        d, gj, xh, xa, a = _group(c, g)
        k1, k2 = c1[s, c.doff:c.doff + C], c2[s, c.doff:c.doff + C]
        dd = a * ((gj - k1) - xh * k2)                               # dL/dd_j;  de[idx_j] += dd_j,  dl = -sum_j dd_j
        ddA = a.abs() * (gj.abs() + k1.abs() + xa * k2.abs())
        tgt = c.nb[g].reshape(-1)
        o.de.index_add_(0, tgt, dd.reshape(-1, C))
        o.deA.index_add_(0, tgt, ddA.reshape(-1, C))
        o.dl[r] = -a * ((SG[r] - k * k1) - k2 * SX[r])
        o.dlA[r] = a.abs() * (SG[r].abs() + k * k1.abs() + k2.abs() * SX[r].abs())
        if dc1 is not None:
            e1, e2 = dc1[s, c.doff:c.doff + C], dc2[s, c.doff:c.doff + C]
            o.de_in.index_add_(0, tgt, (a.abs() * (e1 + xa * e2)).reshape(-1, C))
            o.dl_in[r] = a.abs() * (dSG[r] + k * e1 + k2.abs() * dSX[r] + SX[r].abs() * e2)
        if c.concat:
            gc, xc, xca, ac = _central(c, g)
            o.dl[r] += ac * ((gc - c1[s, :C]) - xc * c2[s, :C])
            o.dlA[r] += ac.abs() * (gc.abs() + c1[s, :C].abs() + xca * c2[s, :C].abs())
            if dc1 is not None:
                o.dl_in[r] += ac.abs() * (dc1[s, :C] + xca * dc2[s, :C])
    o.dl_gate = 2 * (R_DL_CONCAT if c.concat else R_DL) * U * o.dlA
    o.de_gate = 2 * R_DE(o.length.double())[:, None] * U * o.deA               # K per row, from that row's list length
    return o


def ref_end_to_end(c):
    s = ref_sums(c)
    c1, c2, dgamma, dbeta, m = ref_coeffs(c, s.P)
    # what the first two stages may hand the third: their gates, the casts of c1 / c2 included
    setgate = s.P_gate.reshape(c.S, c.gps, c.cbn, 2).sum(1)
    dc1 = setgate[..., 0] / m + 2 * R_CAST * U * c1.abs()
    dc2 = setgate[..., 1] / m + 2 * R_CAST * U * c2.abs()
    f = ref_finish(c, s.SG, s.SX, c1, c2, s.SG_gate, s.SX_gate, dc1, dc2)
    f.dgamma, f.dbeta = dgamma, dbeta
    f.dgamma_gate = setgate[..., 1].sum(0) + 2 * R_CAST * U * dgamma.abs()
    f.dbeta_gate = setgate[..., 0].sum(0) + 2 * R_CAST * U * dbeta.abs()
    return f


def _ratio(got, ref, gate):
    """worst |got - ref| / gate; where the gate is 0 (an empty list: de = 0 exactly) the values must be equal"""
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(err).all())
    assert bool((err[gate == 0] == 0).all())
    return float((err / gate.clamp_min(1e-300)).max()) if err.numel() else 0.0


# ---------------------------------------------------------------------------------------------
# CPU: the reference against autograd, the builder, the launch arithmetic
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [16, 5])
@pytest.mark.parametrize("concat", [1, 0])
def test_edge_backward_closed_form_reference_selftest(concat, k):
    """The closed form, fed float64 statistics, IS float64 autograd of relu(batch_norm(cat[central, e[idx] - l])).mean(k):
    dl, de, dgamma, dbeta to 1e-12 relative (two statistic sets of two groups each)."""
    C, G, Ng, gps = 8, 4, 37, 2
    gen = torch.Generator().manual_seed(k + concat)
    idx = torch.randint(0, Ng, (G, Ng, k), generator=gen)
    c = make_case(C, k, G, Ng, gps, concat, idx, seed=5, dtype=F64, ldg_extra=0)
    f = ref_end_to_end(c)
    LE = c.LE.clone().requires_grad_(True)
    gamma, beta = c.gamma.clone().requires_grad_(True), c.beta.clone().requires_grad_(True)
    loss = 0.0
    for s in range(c.S):
        r = slice(s * gps * Ng, (s + 1) * gps * Ng)
        l = LE[r, :C]
        x = LE[:, C:][c.nb.reshape(c.R, k)[r]] - l[:, None, :]
        if concat:
            x = torch.cat([l[:, None, :].expand(-1, k, -1), x], 2)
        y = F.relu(F.batch_norm(x.permute(2, 0, 1)[None], None, None, gamma, beta, True, 0.1, EPS)).mean(3)
        loss = loss + (y[0].t() * c.gy[r]).sum()
    loss.backward()
    for name, got, want in (("dl", f.dl, LE.grad[:, :C]), ("de", f.de, LE.grad[:, C:]), ("dgamma", f.dgamma, gamma.grad),
                            ("dbeta", f.dbeta, beta.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), name


HUB_CASES = ([(C, 16, G, gps, concat) for C in (32, 64) for concat in (1, 0) for G, gps in ((1, 1), (3, 1), (3, 3))]
             + [(C, k, 3, (3 if concat else 1), concat) for k in (5, 1) for C in (32, 64) for concat in (1, 0)])


def test_index_builder_gives_the_prescribed_in_degrees():
    """every hub case: the wanted lengths exactly (asserted in build_idx from a bincount), an empty list, and the placements
    the kernel's walk distinguishes"""
    for C, k, G, gps, concat in HUB_CASES:
        c = hub_case(C, k, G, gps, concat)
        Q = C // 4
        NG, PPB = 64 // Q, 256 // Q
        deg = torch.bincount(c.nb.reshape(-1), minlength=c.R)
        for g in range(G):
            have = set(int(x) for x in deg[g * c.Ng:(g + 1) * c.Ng])
            assert set(hub_lengths(C, k)) <= have, (C, k, g)
        assert int((c.idx.min())) >= 0 and int(c.idx.max()) < c.Ng           # group-local targets
        hubs = torch.nonzero(deg > HEAD).reshape(-1)
        waves = hubs // NG
        assert bool(((hubs % NG) == 0).any()) and bool(((hubs % NG) == NG - 1).any())
        assert len(set(waves.tolist())) < len(waves)                          # two hubs in one wave
        assert c.R % PPB != 0 and int(deg[c.R - 1]) > HEAD                    # a hub in the block with lanes without a row
        if G > 1:
            assert c.Ng % NG != 0 and (c.Ng - 1) // NG == c.Ng // NG          # rows Ng - 1 and Ng share a wave ...
            assert int(deg[c.Ng - 1]) > HEAD and int(deg[c.Ng]) > HEAD        # ... and both own a tail
        if k == 16:
            assert int(deg.max()) >= 5000


BIG = dict(G=128, Ng=33 * 64 + 5, k=2)


def test_large_shapes_reach_the_tile_loop_and_the_grid_stride(lib_built):
    G, Ng = BIG["G"], BIG["Ng"]
    tiles = -(-Ng // TILE)
    T = pointflow.stat_blocks(G, Ng)
    assert tiles == 34 and T == 17 and T < tiles                              # two tiles per block
    rows = G * Ng
    assert -(-rows // (256 // (64 // 4))) == 16936 > FINISH_CAP               # C = 64: the finish pass strides its grid
    assert -(-rows // (256 // (32 // 4))) <= FINISH_CAP                       # C = 32 does not


# ---------------------------------------------------------------------------------------------
# the three entry points
# ---------------------------------------------------------------------------------------------
def _call(name, *args):
    _lib.call(name, *(list(args) + [_lib.stream()]))
    torch.cuda.synchronize()


def _same_bits(x, y):
    if x is None or y is None:
        return x is y
    as_int = {F32: torch.int32, F64: torch.int64}.get(x.dtype)
    return x.dtype == y.dtype and (torch.equal(x, y) if as_int is None else torch.equal(x.view(as_int), y.view(as_int)))


def _twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert _same_bits(x, y)
    return a


class Device(object):
    """a case's inputs on the device"""

    def __init__(self, dev, c, idx=None):
        self.dev = dev
        self.LE, self.gy_buf = c.LE.to(dev), c.gy_buf.to(dev)
        self.idx = (c.idx if idx is None else idx).contiguous().to(dev)
        self.rows = [r.to(dev) for r in (c.scale, c.shift, c.mean, c.invstd)]


def run_sums(c, d, gy_buf=None, gacc=None, plane=0):
    """-> partials (G, T, cbn, 2) float64 and the rows [sum g | sum xhat] (R, 2C), on the device"""
    T = pointflow.stat_blocks(c.G, c.Ng)
    partials = torch.full((c.G, T, c.cbn, 2), float("nan"), dtype=F64, device=d.dev)
    rows = torch.full((c.R, 2 * c.C), float("nan"), dtype=F32, device=d.dev)
    gy_buf = d.gy_buf if gy_buf is None else gy_buf
    _call("pf_edge_backward_sums_f32", _lib.ptr(d.LE), 2 * c.C, c.C, _lib.ptr(d.idx), c.k, c.G, c.Ng, _lib.ptr(gy_buf),
          int(gy_buf.stride(0)), *([_lib.ptr(r) for r in d.rows] + [c.ld, c.gps, c.concat, _lib.ptr(partials), _lib.ptr(rows),
                                                                     _lib.ptr(gacc), 0 if gacc is None else int(gacc.stride(0)),
                                                                     plane]))
    return partials, rows


def run_coeffs(c, d, partials, into=None):
    """-> c1, c2 (S, cbn), dgamma, dbeta (cbn,)"""
    T = partials.shape[1]
    c1, c2 = [torch.full((c.S, c.cbn), float("nan"), dtype=F32, device=d.dev) for _ in range(2)]
    if into is None:
        dgamma, dbeta = [torch.full((c.cbn,), float("nan"), dtype=F32, device=d.dev) for _ in range(2)]
    else:
        dgamma, dbeta = [t.clone() for t in into]
    _call("pf_edge_backward_coeffs_f32", _lib.ptr(partials), c.G, T, c.cbn, c.C, c.concat, c.gps, c.Ng, c.k, _lib.ptr(c1),
          _lib.ptr(c2), _lib.ptr(dgamma), _lib.ptr(dbeta), 0 if into is None else 1)
    return c1, c2, dgamma, dbeta


def _padded(c, d, x):
    """coefficient rows (S, cbn) in the affine rows' leading dimension (the finish pass reads all six with one ld)"""
    if c.ld == c.cbn:
        return x
    out = torch.full((c.S, c.ld), float("nan"), dtype=F32, device=d.dev)
    out[:, :c.cbn] = x
    return out


def run_finish(c, d, sums_rows, c1, c2, order, start, gy_buf=None, plane=0):
    """-> [dl | de] (R, 2C); sums_rows is not modified"""
    dle = sums_rows.clone()
    gy_buf = d.gy_buf if gy_buf is None else gy_buf
    p1, p2 = _padded(c, d, c1), _padded(c, d, c2)                       # (named: they must outlive the call)
    _call("pf_edge_backward_finish_f32", _lib.ptr(d.LE), 2 * c.C, c.C, c.k, c.G, c.Ng, _lib.ptr(gy_buf), int(gy_buf.stride(0)),
          *([_lib.ptr(r) for r in d.rows] + [_lib.ptr(p1), _lib.ptr(p2), c.ld, c.gps, c.concat, _lib.ptr(dle), _lib.ptr(order),
                                             _lib.ptr(start), plane]))
    return (dle,)


def check_inverse(c, order, start):
    """pf_knn_inverse's lists = a stable host argsort of the clamped keys"""
    keys = c.nb.reshape(-1).numpy()
    want_order = np.argsort(keys, kind="stable")
    want_start = np.searchsorted(keys[want_order], np.arange(c.R + 1), side="left")
    assert np.array_equal(start.cpu().numpy().astype(np.int64) & 0xffffffff, want_start)
    assert np.array_equal(order.cpu().numpy().astype(np.int64) & 0xffffffff, want_order)


def check_stages(dev, c, name, stages=("sums", "coeffs", "finish", "composed")):
    """the three entry points, each against float64 given the previous one's actual output, and their composition"""
    d = Device(dev, c)
    out = {}
    partials, rows = _twice(lambda: run_sums(c, d))
    if "sums" in stages:
        s = ref_sums(c)
        got = partials.cpu().sum(1)
        out["partials_g"] = _ratio(got[..., 0], s.P[..., 0], s.P_gate[..., 0])
        out["partials_gx"] = _ratio(got[..., 1], s.P[..., 1], s.P_gate[..., 1])
        out["row_sum_g"] = _ratio(rows.cpu()[:, :c.C], s.SG, s.SG_gate)
        out["row_sum_xhat"] = _ratio(rows.cpu()[:, c.C:], s.SX, s.SX_gate)
    c1, c2, dgamma, dbeta = _twice(lambda: run_coeffs(c, d, partials))
    if "coeffs" in stages:
        pk = partials.cpu()
        w1, w2, wg, wb, m = ref_coeffs(c, pk.sum(1))
        # one cast each; the float64 additions of the T * gps (then S) partial rows, either side
        n64 = 2 * (pk.shape[1] * c.gps + c.S) * U64
        setA = pk.abs().sum(1).reshape(c.S, c.gps, c.cbn, 2).sum(1)
        out["c1"] = _ratio(c1.cpu(), w1, (2 * R_CAST * U + n64) * setA[..., 0] / m)
        out["c2"] = _ratio(c2.cpu(), w2, (2 * R_CAST * U + n64) * setA[..., 1] / m)
        out["dgamma"] = _ratio(dgamma.cpu(), wg, (2 * R_CAST * U + n64) * setA[..., 1].sum(0))
        out["dbeta"] = _ratio(dbeta.cpu(), wb, (2 * R_CAST * U + n64) * setA[..., 0].sum(0))
    order, start = pointflow.knn_inverse(d.idx, c.G, c.Ng, c.k)
    torch.cuda.synchronize()
    check_inverse(c, order, start)
    (dle,) = _twice(lambda: run_finish(c, d, rows, c1, c2, order, start))
    dle = dle.cpu()
    if "finish" in stages:
        f = ref_finish(c, rows.cpu()[:, :c.C].double(), rows.cpu()[:, c.C:].double(), c1.cpu().double(), c2.cpu().double())
        out["dl"] = _ratio(dle[:, :c.C], f.dl, f.dl_gate)
        out["de"] = _ratio(dle[:, c.C:], f.de, f.de_gate)
        out["longest_list"] = float(f.length.max())
    if "composed" in stages:
        e = ref_end_to_end(c)
        out["composed_dl"] = _ratio(dle[:, :c.C], e.dl, e.dl_gate + e.dl_in)
        out["composed_de"] = _ratio(dle[:, c.C:], e.de, e.de_gate + e.de_in)
        out["composed_dgamma"] = _ratio(dgamma.cpu(), e.dgamma, e.dgamma_gate)
        out["composed_dbeta"] = _ratio(dbeta.cpu(), e.dbeta, e.dbeta_gate)
    print(name, out)
    report(name, **out)
    worst = max(v for q, v in out.items() if q != "longest_list")
    assert worst <= 1.0, out
    assert _lib.status() == 0
    return partials, rows, c1, c2, dgamma, dbeta, dle


@gpu
@pytest.mark.parametrize("C,k,G,gps,concat", HUB_CASES)
def test_edge_backward_hub_lists_kernel_by_kernel(dev, C, k, G, gps, concat):
    """Prescribed in-degrees (hub_lengths, hub_layout) through sums, coeffs and finish: k = 16 takes
    edge_bwd_reduce_kernel<C, 16> and the p >> 4 arm, k = 5 and k = 1 the runtime-k kernel and p / k; G = 3 puts two tail
    owners of different groups in one wave (the `!same` arm) and, with groups_per_stat 1, three sets of affine rows in a
    leading dimension wider than the BatchNorm; groups_per_stat 3 pools them."""
    c = hub_case(C, k, G, gps, concat)
    check_stages(dev, c, "edge_bwd_hubs_C%d_k%d_G%d_gps%d_concat%d" % (C, k, G, gps, concat))


@functools.lru_cache(maxsize=None)
def big_case(C, concat):
    G, Ng, k = BIG["G"], BIG["Ng"], BIG["k"]
    gen = torch.Generator().manual_seed(C)
    idx = torch.randint(0, Ng, (G, Ng, k), generator=gen)
    NG = 64 // (C // 4)
    idx[G - 1] = build_idx(Ng, k, {Ng - 1: HEAD + 4 * NG + 1, 7: HEAD + 1}, [3], seed=C)
    return make_case(C, k, G, Ng, 4, concat, idx, seed=C + 1)


@gpu
def test_edge_passes_walk_several_tiles_per_block(dev):
    """G = 128 groups of 33 * 64 + 5 points: 34 tiles on T = 17 blocks per group, the `tile += T` trip of the reduce pass
    and of pf_edge_stats_f32 / pf_edge_apply_f32 (k = 2: the runtime-k kernels), 32 statistic sets of 4 groups."""
    c = big_case(32, 1)
    C, k, G, Ng = c.C, c.k, c.G, c.Ng
    T = pointflow.stat_blocks(G, Ng)
    assert T < -(-Ng // TILE)
    check_stages(dev, c, "edge_bwd_tiles_C32", stages=("sums",))
    d = Device(dev, c)

    def stats():
        p = torch.full((G, T, C, 2), float("nan"), dtype=F64, device=dev)
        _call("pf_edge_stats_f32", _lib.ptr(d.LE), 2 * C, C, _lib.ptr(d.idx), k, G, Ng, _lib.ptr(p), None, 0, 0, 0)
        return (p,)

    def apply():
        y = torch.full((c.R, c.cbn + 4), float("nan"), dtype=F32, device=dev)
        _call("pf_edge_apply_f32", _lib.ptr(d.LE), 2 * C, C, _lib.ptr(d.idx), k, G, Ng, _lib.ptr(d.rows[0]), _lib.ptr(d.rows[1]),
              c.ld, c.gps, c.concat, _lib.ptr(y), c.cbn + 4, None, 0, 0, 0)
        return (y,)

    (p,), (y,) = _twice(stats), _twice(apply)
    p, y = p.cpu().sum(1), y.cpu()
    assert bool(torch.isnan(y[:, c.cbn:]).all())
    want_p, A_p = torch.zeros(G, C, 2, dtype=F64), torch.zeros(G, C, 2, dtype=F64)
    want_y, A_y = torch.zeros(c.R, c.cbn, dtype=F64), torch.zeros(c.R, c.cbn, dtype=F64)
    for g in range(G):
        r = slice(g * Ng, (g + 1) * Ng)
        dd = _group(c, g)[0]
        want_p[g, :, 0], A_p[g, :, 0] = dd.sum((0, 1)), dd.abs().sum((0, 1))
        want_p[g, :, 1] = A_p[g, :, 1] = (dd * dd).sum((0, 1))
        a, b, _, _ = _aff(c, g, c.doff)
        u = dd * a + b
        want_y[r, c.doff:], A_y[r, c.doff:] = u.clamp_min(0).sum(1) / k, ((u > 0) * ((dd * a).abs() + b.abs())).sum(1) / k
        l = c.LE[r, :C].double()
        a, b, _, _ = _aff(c, g, 0)
        want_y[r, :C], A_y[r, :C] = (l * a + b).clamp_min(0), ((l * a + b) > 0) * ((l * a).abs() + b.abs())
    # stats: s += d (k - 1 roundings; d itself is the reference's), s2 += d * d (1 + k - 1); then float64
    Kp = torch.tensor([2.0 * (k - 1), 2.0 * k], dtype=F64)
    # apply: fmaf (1), a += . (k - 1), a / kf (1); central: fmaf (1)
    Ky = torch.cat([torch.full((C,), 2.0 * 1, dtype=F64), torch.full((C,), 2.0 * (k + 1), dtype=F64)])
    out = dict(stats=_ratio(p, want_p, (Kp * U + 2 * Ng * k * U64) * A_p), apply=_ratio(y[:, :c.cbn], want_y, Ky * U * A_y))
    print(out)
    report("edge_fwd_tiles_C32", **out)
    assert max(out.values()) <= 1.0, out
    assert _lib.status() == 0


@gpu
def test_edge_backward_finish_strides_its_grid(dev):
    """The same rows at C = 64: 16 936 row groups on 16 384 blocks, the finish pass's second trip (a hub tail on the last
    row, which only that trip reaches), from the kernels' own sums and coefficients."""
    c = big_case(64, 0)
    assert -(-c.R // (256 // (c.C // 4))) > FINISH_CAP
    check_stages(dev, c, "edge_bwd_grid_stride_C64", stages=("finish",))


@gpu
@pytest.mark.parametrize("concat", [1, 0])
def test_edge_backward_grad_acc_is_the_float32_sum_and_holds_it(dev, concat):
    """grad_acc: the bits of a call that is handed grad_y + grad_acc (a float32 sum) as grad_y, through the wrapper; afterwards
    grad_acc holds that sum."""
    c = hub_case(64, 5, 3, (3 if concat else 1), concat)
    d = Device(dev, c)
    gen = torch.Generator().manual_seed(11)
    h = torch.randn(c.R, c.cbn, generator=gen)
    total = (c.gy + h).contiguous()
    keep = dict(LE=d.LE, scale=d.rows[0][:, :c.cbn].contiguous(), shift=d.rows[1][:, :c.cbn].contiguous(),
                mean=d.rows[2][:, :c.cbn].contiguous(), invstd=d.rows[3][:, :c.cbn].contiguous())
    args = (c.C, c.k, c.G, c.Ng, c.gps, c.concat)

    def with_acc():
        acc = h.to(dev)
        out = pointflow.edge_conv_backward(keep, d.idx, d.gy_buf[:, :c.cbn], *args, grad_acc=acc)
        torch.cuda.synchronize()
        return list(out) + [acc]

    def summed():
        out = pointflow.edge_conv_backward(keep, d.idx, total.to(dev), *args)
        torch.cuda.synchronize()
        return list(out)

    a, b = _twice(with_acc), _twice(summed)
    assert torch.equal(a[3].cpu(), total)
    for x, y in zip(a[:3], b):
        assert torch.equal(x, y)
    assert _lib.status() == 0


@gpu
def test_edge_backward_coeffs_into_adds_to_what_is_there(dev):
    c = hub_case(32, 5, 3, 3, 1)
    d = Device(dev, c)
    partials, _ = run_sums(c, d)
    c1, c2, dgamma, dbeta = _twice(lambda: run_coeffs(c, d, partials))
    gen = torch.Generator().manual_seed(12)
    old = [torch.randn(c.cbn, generator=gen).to(dev) for _ in range(2)]
    a1, a2, agamma, abeta = _twice(lambda: run_coeffs(c, d, partials, into=old))
    assert torch.equal(a1, c1) and torch.equal(a2, c2)
    assert torch.equal(agamma.cpu(), old[0].cpu() + dgamma.cpu()) and torch.equal(abeta.cpu(), old[1].cpu() + dbeta.cpu())
    assert _lib.status() == 0


@gpu
@pytest.mark.parametrize("C", [32, 64])
def test_edge_backward_plane_hint_is_a_pure_relabelling(dev, C):
    """G = 1, 1024 points, plane 512: 8 (sums), 16 or 32 (finish) row groups per plane, a multiple of 8 of whole units and
    one per block -- band > 0 in both passes; the bits of plane 0."""
    k, Ng, plane = 16, 1024, 512
    Q = C // 4
    NG = 64 // Q
    assert pointflow.stat_blocks(1, Ng) == Ng // TILE and (plane // TILE) % 8 == 0 and Ng % plane == 0
    assert (plane // (256 // Q)) % 8 == 0 and Ng // (256 // Q) <= FINISH_CAP
    idx = build_idx(Ng, k, {0: 1003, NG - 1: HEAD + 8 * NG + 3, 517: HEAD + 1, Ng - 1: HEAD + NG}, [5, 600], seed=C)
    c = make_case(C, k, 1, Ng, 1, 1, idx, seed=C + 2)
    d = Device(dev, c)
    p0, r0 = _twice(lambda: run_sums(c, d))
    p1, r1 = _twice(lambda: run_sums(c, d, plane=plane))
    assert torch.equal(p0, p1) and torch.equal(r0, r1)
    c1, c2, _, _ = run_coeffs(c, d, p0)
    order, start = pointflow.knn_inverse(d.idx, 1, Ng, k)
    (f0,) = _twice(lambda: run_finish(c, d, r0, c1, c2, order, start))
    (f1,) = _twice(lambda: run_finish(c, d, r0, c1, c2, order, start, plane=plane))
    assert torch.equal(f0, f1)
    assert _lib.status() == 0


@gpu
@pytest.mark.parametrize("k", [16, 5])
def test_edge_backward_clamps_bad_indices_like_the_inverse(dev, k):
    """a few of -1, Ng, Ng + 7: the forward walk and pf_knn_inverse clamp alike, so every gradient has the bits of the call
    with idx clamped to [0, Ng - 1]; the bad-index bit is reported once, then 0."""
    c = hub_case(32, k, 3, 1, 1)
    bad = c.idx.clone()
    at_low, at_high = torch.nonzero(bad == 0), torch.nonzero(bad == c.Ng - 1)
    assert len(at_low) >= 3 and len(at_high) >= 4
    for g, n, j in at_low[:3].tolist():
        bad[g, n, j] = -1
    for i, (g, n, j) in enumerate(at_high[:4].tolist()):
        bad[g, n, j] = c.Ng + 7 * (i % 2)
    assert torch.equal(bad.clamp(0, c.Ng - 1), c.idx) and int((bad != c.idx).sum()) == 7
    good_d, bad_d = Device(dev, c), Device(dev, c, idx=bad)
    assert _lib.status() == 0

    def chain(d):
        partials, rows = _twice(lambda: run_sums(c, d))
        c1, c2, dgamma, dbeta = _twice(lambda: run_coeffs(c, d, partials))
        order, start = pointflow.knn_inverse(d.idx, c.G, c.Ng, c.k)
        torch.cuda.synchronize()
        check_inverse(c, order, start)
        return [partials, rows, c1, c2, dgamma, dbeta, _twice(lambda: run_finish(c, d, rows, c1, c2, order, start))[0]]

    got = chain(bad_d)
    assert _lib.status() & 1
    assert _lib.status() == 0
    want = chain(good_d)
    assert _lib.status() == 0
    for x, y in zip(got, want):
        assert torch.equal(x, y)


@gpu
def test_edge_backward_empty_problem_touches_nothing(dev):
    c = hub_case(32, 1, 3, 1, 0)
    d = Device(dev, c)
    for G, Ng in ((0, c.Ng), (c.G, 0)):
        partials = torch.full((4, c.cbn, 2), -7.0, dtype=F64, device=dev)
        rows = torch.full((16, 2 * c.C), -7.0, dtype=F32, device=dev)
        acc = torch.full((16, c.cbn), -7.0, dtype=F32, device=dev)
        r = [_lib.ptr(x) for x in d.rows]
        _call("pf_edge_backward_sums_f32", _lib.ptr(d.LE), 2 * c.C, c.C, _lib.ptr(d.idx), c.k, G, Ng, _lib.ptr(d.gy_buf), c.ldg,
              *(r + [c.ld, 1, c.concat, _lib.ptr(partials), _lib.ptr(rows), _lib.ptr(acc), c.cbn, 0]))
        _call("pf_edge_backward_finish_f32", _lib.ptr(d.LE), 2 * c.C, c.C, c.k, G, Ng, _lib.ptr(d.gy_buf), c.ldg,
              *(r + [_lib.ptr(rows), _lib.ptr(rows), c.ld, 1, c.concat, _lib.ptr(rows), None, None, 0]))
        _call("pf_knn_inverse", _lib.ptr(d.idx), c.k, G, Ng, _lib.ptr(rows), _lib.ptr(rows), None, 0)
        for x in (partials, rows, acc):
            assert bool((x == -7.0).all())
    assert _lib.status() == 0


@gpu
def test_edge_backward_argument_rejections(dev):
    """the PF_REQUIRE lines of the three entry points, one argument wrong at a time on an otherwise valid call (nothing is
    launched); C = 128 is unsupported in the backward"""
    c = hub_case(32, 1, 3, 1, 1)
    d = Device(dev, c)
    T = pointflow.stat_blocks(c.G, c.Ng)
    partials = torch.zeros((c.G, T, c.cbn, 2), dtype=F64, device=dev)
    rows = torch.zeros((c.R, 2 * c.C), dtype=F32, device=dev)
    co = torch.zeros((c.S, c.ld), dtype=F32, device=dev)
    order, start = pointflow.knn_inverse(d.idx, c.G, c.Ng, c.k)
    r = [_lib.ptr(x) for x in d.rows]
    P = _lib.ptr

    def sums(ldle=2 * c.C, C=c.C, idx=d.idx, k=c.k, G=c.G, Ng=c.Ng, gy=d.gy_buf, ldg=c.ldg, scale=d.rows[0], ld=c.ld, gps=c.gps,
             part=partials, gle=rows, acc=None, lda=0, plane=0):
        _call("pf_edge_backward_sums_f32", P(d.LE), ldle, C, P(idx), k, G, Ng, P(gy), ldg, P(scale), r[1], r[2], r[3], ld, gps,
              c.concat, P(part), P(gle), P(acc), lda, plane)

    def coeffs(part=partials, G=c.G, T=T, cbn=c.cbn, C=c.C, gps=c.gps, Ng=c.Ng, k=c.k, c1=co):
        _call("pf_edge_backward_coeffs_f32", P(part), G, T, cbn, C, c.concat, gps, Ng, k, P(c1), P(co), None, None, 0)

    def finish(ldle=2 * c.C, C=c.C, k=c.k, G=c.G, ldg=c.ldg, c1=co, ld=c.ld, gps=c.gps, gle=rows, order=order, start=start,
               plane=0):
        _call("pf_edge_backward_finish_f32", P(d.LE), ldle, C, k, G, c.Ng, P(d.gy_buf), ldg, r[0], r[1], r[2], r[3], P(c1), P(co),
              ld, gps, c.concat, P(gle), P(order), P(start), plane)

    acc = torch.zeros((c.R, c.cbn), dtype=F32, device=dev)
    invalid = [
        lambda: sums(ldle=2 * c.C - 4), lambda: sums(ldle=2 * c.C + 2), lambda: sums(k=0), lambda: sums(G=-1), lambda: sums(Ng=-1),
        lambda: sums(G=65536), lambda: sums(ldg=c.ldg + 2), lambda: sums(ldg=c.cbn - 4), lambda: sums(ld=c.cbn - 4),
        lambda: sums(ld=c.cbn + 2), lambda: sums(gps=0), lambda: sums(plane=-1), lambda: sums(gle=None), lambda: sums(idx=None),
        lambda: sums(gy=None), lambda: sums(scale=None), lambda: sums(part=None), lambda: sums(acc=acc, lda=c.cbn - 4),
        lambda: sums(acc=acc, lda=c.cbn + 2),
        lambda: coeffs(G=0), lambda: coeffs(T=0), lambda: coeffs(gps=2), lambda: coeffs(gps=0), lambda: coeffs(cbn=c.C),
        lambda: coeffs(Ng=0), lambda: coeffs(k=0), lambda: coeffs(part=None), lambda: coeffs(c1=None),
        lambda: finish(ldle=2 * c.C - 4), lambda: finish(ldle=2 * c.C + 2), lambda: finish(k=0), lambda: finish(G=-1),
        lambda: finish(ldg=c.ldg + 2), lambda: finish(ldg=c.cbn - 4), lambda: finish(ld=c.cbn - 4), lambda: finish(ld=c.cbn + 2),
        lambda: finish(gps=0), lambda: finish(plane=-1), lambda: finish(c1=None), lambda: finish(gle=None),
        lambda: finish(order=None), lambda: finish(start=None),
    ]
    for i, f in enumerate(invalid):
        with pytest.raises(RuntimeError, match="invalid argument"):
            f()
            pytest.fail("call %d was accepted" % i)
    for f in (lambda: sums(C=128, ldle=256, ld=256, ldg=256), lambda: finish(C=128, ldle=256, ld=256, ldg=256)):
        with pytest.raises(RuntimeError, match="unsupported"):
            f()
    sums()                                                               # the unmodified calls are accepted
    coeffs()
    finish()
    assert bool((partials == 0).sum() < partials.numel())
    assert _lib.status() == 0
