"""The forward side of the warp family kernel by kernel through the C ABI and the thin wrappers: csrc/fetch.hip
(pf_fetch_forward / backward / variance, pf_frustum_variance planar and channel-last, pf_nchw_to_nhwc, pf_flow_features) and
the inference head pf_flow_head_f32 (csrc/edgeconv.hip), each against a float64 evaluation of the formula its comment states.

As in tests/test_gpu_warp_bwd.py (whose scene builders and formula helpers this file imports) the reference of a VALUE check
never projects on its own terms: on the exact scene (identity rotations, power-of-two focals and depth planes, dyadic
translations, the 17 x 33 map) a float32 and a float64 evaluation of wb_world + pf_project_taps give the same keys and
fractional offsets bit for bit -- asserted on the CPU before every use -- so both sides read the same four texels with the
same weights and the gate is float32 rounding of the arithmetic alone,
    |got - ref| <= K * 2^-24 * A,
A = the reference expression with every product and term replaced by its absolute value, K = twice the float32 roundings on
the kernel's path (counted where each gate is built).  Every test reports its worst |got - ref| / (K 2^-24 A) next to K.
Layout properties (sub-grid order, nearest resize of the prior) are checked bit for bit against the ratio-1 call on generic
cameras: the arithmetic is per pixel, a difference is an indexing error.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import report
from pointmvsnet_amd import _lib, pointflow
from pointmvsnet_amd.utils import feature_fetcher
from test_gpu_warp_bwd import (F64, NOKEY, U, _EH, _EW, _assert_exact_scene_covers_the_edges, _cam_block, _exact_reference,
                               _exact_scene, _generic_scene, _project, _world)

pytestmark = pytest.mark.gpu

F32 = torch.float32
NAN = float("nan")
SENT = -7777.25                                     # fill of the guard tail behind every output buffer
GUARD = 1024
PF_ERR_INVALID_ARG, PF_ERR_UNSUPPORTED = -1, -2


def _call(name, *args):
    _lib.call(name, *(list(args) + [_lib.stream()]))
    torch.cuda.synchronize()


def _raw(name, *args):
    """the entry point's return code (no exception)"""
    code = getattr(_lib.load(), name)(*(list(args) + [_lib.stream()]))
    torch.cuda.synchronize()
    return int(code)


def _guarded(n, dev, fill=NAN):
    """n floats of `fill` and a guard tail of SENT behind them, on the device"""
    buf = torch.full((n + GUARD,), fill, dtype=F32)
    buf[n:] = SENT
    return buf.to(dev)


def _take(buf, n, what):
    """the n floats of a _guarded buffer on the CPU; nothing behind them was written"""
    host = buf.cpu()
    assert bool((host[n:] == SENT).all()), "%s: written beyond its %d elements" % (what, n)
    return host[:n]


def _gate(got, ref, A, K, what):
    """|got - ref| <= K 2^-24 A everywhere (0 where A is 0); returns the worst |got - ref| / (K 2^-24 A)"""
    got = got.double()
    assert bool(torch.isfinite(got).all()), (what, "not finite")
    err = (got - ref).abs()
    bound = K * U * A
    pos = A > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    print("%s: worst |got - ref| / (K u A) = %.4f, K = %s" % (what, ratio, K if isinstance(K, (int, float)) else "per element"))
    assert bool((err <= bound).all()), (what, "ratio to gate", ratio)
    return ratio


# ---------------------------------------------------------------------------------------------
# the four taps and the bilinear sum from (key, fxy) in a dtype of choice
# ---------------------------------------------------------------------------------------------
def _taps(dtype, keys, fxy, H, W):
    """keys (V, N) int64, fxy (V, N, 2) -> texel offsets (4, V, N) and weights (4, V, N) in `dtype`, order nw, ne, sw, se;
    weight 0 (and offset 0) for a tap outside the map and for a pair without a key, whatever fxy holds there (NaN too)"""
    V = keys.shape[0]
    cells = (H + 1) * (W + 1)
    keyed = keys != NOKEY
    cell = torch.where(keyed, keys - torch.arange(V).view(V, 1) * cells, torch.zeros_like(keys))
    assert bool(((cell >= 0) & (cell < cells)).all())
    yi, xi = torch.div(cell, W + 1, rounding_mode="floor") - 1, cell % (W + 1) - 1
    fx, fy = fxy[..., 0].to(dtype), fxy[..., 1].to(dtype)
    offs, wgts = [], []
    for k in range(4):
        ty, tx = yi + (k >> 1), xi + (k & 1)
        ok = keyed & (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
        w = (fy if k >> 1 else 1.0 - fy) * (fx if k & 1 else 1.0 - fx)
        offs.append(torch.where(ok, ty * W + tx, torch.zeros_like(ty)))
        wgts.append(torch.where(ok, w, torch.zeros_like(w)))
    return torch.stack(offs), torch.stack(wgts)


def _sample(dtype, texels, keys, fxy, H, W):
    """texels (V, H * W, C) -> f, fa (V, N, C) in `dtype`: f = ((nw a + ne b) + sw c) + se d, taps outside the map
    contributing zero; fa the same with every product replaced by its absolute value"""
    off, wgt = _taps(dtype, keys, fxy, H, W)
    V, N = keys.shape
    texels = texels.to(dtype)
    f, fa = [], []
    for v in range(V):
        t = [texels[v][off[k, v]] * wgt[k, v].view(N, 1) for k in range(4)]
        f.append(((t[0] + t[1]) + t[2]) + t[3])
        fa.append(((t[0].abs() + t[1].abs()) + t[2].abs()) + t[3].abs())
    return torch.stack(f), torch.stack(fa)


def _variance(f, fa):
    """views in ascending order, E[f^2] - E[f]^2; A = E[fa^2] + E[fa]^2"""
    V = f.shape[0]
    s, s2 = f[0].clone(), f[0] * f[0]
    sa, s2a = fa[0].clone(), fa[0] * fa[0]
    for v in range(1, V):
        s, s2 = s + f[v], s2 + f[v] * f[v]
        sa, s2a = sa + fa[v], s2a + fa[v] * fa[v]
    return s2 / V - (s / V) * (s / V), s2a / V + (sa / V) * (sa / V)


# Roundings of the variance kernels (fetch.hip) on the path of one output, K_VAR(V) = 2 (2 V + 17):
#   a tap weight: 1 - fx, 1 - fy, their product (3); pf_bilerp: a product and three fmaf (4) -> f carries 7
#   s : V - 1 additions -> 7 + V - 1;  m1 = s * inv_v with inv_v = 1 / V rounded (2) -> V + 8;  m1 * m1 doubles it: 2 V + 16
#   s2: f * f doubles f's 7 -> 14, one rounding per view (V), inv_v and the product s2 * inv_v (2) -> V + 16
#   the closing fmaf of pf_variance: 1 -> the longer path has 2 V + 17.
def K_VAR(V):
    return 2 * (2 * V + 17)


def _exact_taps(points_of, K, E, H, W, keyed_only=False):
    """keys, fxy of pf_project_taps in float64 -- after the assertion of _exact_reference: a float32 evaluation of the same
    formulas gives them bit for bit.  keyed_only: the offsets are compared where the pair has a key (points that no
    projection can place carry NaN / inf offsets on both sides)"""
    r32 = _project(F32, points_of(F32), K, E, H, W)
    r64 = _project(F64, points_of(F64), K, E, H, W)
    assert torch.equal(r32[0], r64[0])
    if keyed_only:
        keyed = r64[0] != NOKEY
        assert torch.equal(r32[1].double()[keyed], r64[1][keyed])
    else:
        assert torch.equal(r32[1].double(), r64[1])
    return r64[0], r64[1]


def _covers_the_edges(keys, fxy, V, H, W):
    """_assert_exact_scene_covers_the_edges; its border cells xi = -1 / yi = -1 and the strictly inside points come with the
    third view, so with two views the assertions are view 0's (texel centres, the cells xi = W - 1 and yi = H - 1) and that
    view 1 puts points outside the map"""
    if V == 2:
        _assert_exact_scene_covers_the_edges(keys[:1], fxy[:1], 1, H, W)
        assert bool((keys[1] == NOKEY).any())
    else:
        _assert_exact_scene_covers_the_edges(keys, fxy, V, H, W)


def _texels(maps):
    """(V, C, H, W) -> (V, H * W, C) float64"""
    V, C, H, W = maps.shape
    return maps.permute(0, 2, 3, 1).reshape(V, H * W, C).double()


# ---------------------------------------------------------------------------------------------
# 1. values on the exact scene
# ---------------------------------------------------------------------------------------------
_IDENT_E = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])


@functools.lru_cache(maxsize=None)
def _fetch_scene(V):
    """the world points of the frustum (256, 512, 1024) of the exact scene and their taps in the V views, with the scene's
    extrinsics and with E = NULL (the identity: the points are taken as camera coordinates of every view)"""
    H, W = _EH, _EW
    (kinv, rinv, t, K, E, depths), k64, f64 = _exact_reference(V, flow=False)
    _covers_the_edges(k64, f64, V, H, W)
    pts_of = lambda dt: _world(dt, kinv, rinv, t, depths.to(dt).repeat_interleave(H * W), H, W)      # noqa: E731
    pts = torch.stack(pts_of(F64))
    assert torch.equal(pts.float().double(), pts)                                  # the points are float32 numbers
    kE, fE = _exact_taps(pts_of, K, E, H, W)
    assert torch.equal(kE, k64) and torch.equal(fE, f64)
    k0, f0 = _exact_taps(pts_of, K, _IDENT_E.repeat(V, 1), H, W)
    return K, E, pts, {True: (kE, fE), False: (k0, f0)}


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("V", [1, 3, 8])
def test_fetch_forward_exact_scene_vs_float64(dev, V, C):
    """pf_fetch_forward_f32 (pf_sample: four separate products, three additions) on the exact scene, E given and E = NULL.
    Roundings on the path of one term: 1 - fx, 1 - fy, the weight product (3), the product with the texel (1), the three
    additions (3): 7 -> K = 14.  A second map holds integers in [-4, 4]: the weights are dyadic with at most 14 bits, so a
    float32 evaluation of the formula equals the float64 one (asserted per view on the CPU) and the kernel must give those
    bits; a view for which the CPU assertion fails keeps the gate."""
    H, W = _EH, _EW
    Kc, E, pts, taps = _fetch_scene(V)
    N = pts.shape[1]
    g = torch.Generator().manual_seed(1000 * V + C)
    maps = torch.randn((1, V, C, H, W), generator=g)
    ints = torch.randint(-4, 5, (1, V, C, H, W), generator=g).float()
    d_pts, d_K, d_E = pts.float().view(1, 3, N).to(dev), Kc.view(1, V, 9).to(dev), E.view(1, V, 12).to(dev)
    worst, exact_views = 0.0, 0
    for with_E in (True, False):
        keys, fxy = taps[with_E]
        for m, integer in ((maps, False), (ints, True)):
            out, d_m = _guarded(V * C * N, dev), m.to(dev)
            _call("pf_fetch_forward_f32", _lib.ptr(d_m), _lib.ptr(d_pts), _lib.ptr(d_K),
                  _lib.ptr(d_E) if with_E else None, _lib.ptr(out), 1, V, C, H, W, N)
            got = _take(out, V * C * N, "fetch_forward").view(V, C, N).permute(0, 2, 1)
            f, fa = _sample(F64, _texels(m[0]), keys, fxy, H, W)
            worst = max(worst, _gate(got, f, fa, 14, "fetch_forward V%d C%d E%d int%d" % (V, C, with_E, integer)))
            if integer:
                f32, _ = _sample(F32, _texels(m[0]), keys, fxy, H, W)
                for v in range(V):
                    if torch.equal(f32[v].double(), f[v]) and torch.equal(f[v].float().double(), f[v]):
                        exact_views += 1
                        assert torch.equal(got[v].double(), f[v]), ("integer map: bits differ", V, C, with_E, v)
    # (measured on the CPU: the assertion holds for every view of the scene -- no view falls back to the gate)
    assert exact_views == 2 * V, exact_views
    report("fetch_forward_exact_V%d_C%d" % (V, C), ratio_to_gate=worst, K=14, bit_exact_views=exact_views)


@pytest.mark.parametrize("V", [1, 3, 8])
def test_fetch_backward_exact_scene_vs_float64_scatter(dev, V):
    """pf_fetch_backward_f32 on the same points with a random grad_out, against an order-free float64 scatter-add; C = 5,
    E given and E = NULL.  Per texel A = sum |g| |w|; roundings: 1 - fx, 1 - fy, the weight product (3), the product with g
    (1), one addition per term of the longest list that hits the texel -> K = 2 (terms + 4).  A texel no tap touches is
    exactly 0."""
    H, W, C = _EH, _EW, 5
    Kc, E, pts, taps = _fetch_scene(V)
    N = pts.shape[1]
    g = torch.Generator().manual_seed(2000 + V)
    gout = torch.randn((1, V, C, N), generator=g)
    d_pts, d_K, d_E = pts.float().view(1, 3, N).to(dev), Kc.view(1, V, 9).to(dev), E.view(1, V, 12).to(dev)
    d_gout = gout.to(dev)
    worst, longest = 0.0, 0.0
    for with_E in (True, False):
        keys, fxy = taps[with_E]
        off, wgt = _taps(F64, keys, fxy, H, W)
        tex = (off + torch.arange(V).view(1, V, 1) * (H * W)).reshape(4, -1)                 # rows of (V * H * W, C)
        gv = gout[0].permute(0, 2, 1).reshape(V * N, C).double()
        ref = torch.zeros((V * H * W, C), dtype=F64)
        A = torch.zeros((V * H * W, C), dtype=F64)
        terms = torch.zeros(V * H * W, dtype=F64)
        for k in range(4):
            ref.index_add_(0, tex[k], gv * wgt[k].reshape(-1, 1))
            A.index_add_(0, tex[k], gv.abs() * wgt[k].reshape(-1, 1))
            terms.index_add_(0, tex[k], (wgt[k].reshape(-1) != 0).double())
        out = _guarded(V * C * H * W, dev, fill=12345.678)                                  # the entry point clears it
        _call("pf_fetch_backward_f32", _lib.ptr(d_gout), _lib.ptr(d_pts), _lib.ptr(d_K),
              _lib.ptr(d_E) if with_E else None, _lib.ptr(out), 1, V, C, H, W, N)
        got = _take(out, V * C * H * W, "fetch_backward").view(V, C, H * W).permute(0, 2, 1).reshape(V * H * W, C)
        untouched = terms == 0
        assert bool((got[untouched] == 0).all())
        if with_E and V == 8:                                         # (the first three views cover their maps; views 3 .. 7 do not)
            assert bool(untouched.any())
        Kt = (2.0 * (terms + 4.0)).view(-1, 1)
        err = (got.double() - ref).abs()
        bound = Kt * U * A
        pos = A > 0
        worst = max(worst, float((err[pos] / bound.expand_as(A)[pos]).max()))
        longest = max(longest, float(terms.max()))
        assert bool((err <= bound).all()), (V, with_E, worst)
    report("fetch_backward_exact_V%d" % V, ratio_to_gate=worst, longest_list_terms=longest, K=2 * (longest + 4))


_CMAX = 68
_COARSE_DEPTHS = torch.tensor([[256.0, 512.0, 1024.0], [2048.0, 128.0, 512.0]])


@functools.lru_cache(maxsize=None)
def _coarse_reference(V):
    """B = 2 items of the exact scene, 68-channel maps (the tests take the first C channels): item 0 is _exact_reference's
    scene, item 1 has the views in reverse order and the depth planes (2048, 128, 512) -- powers of two, so the scene
    stays exact (the same assertion).  Returns the inputs and, per ref_override, the float64 variance and its A,
    (B, N, 68), plus the float64 world points (B, 3, N)."""
    H, W = _EH, _EW
    kinv, rinv, t, K, E = _exact_scene(V, flow=False)
    _, k_ref, f_ref = _exact_reference(V, flow=False)
    g = torch.Generator().manual_seed(3000 + V)
    maps = torch.randn((2, V, _CMAX, H, W), generator=g)
    Kb, Eb, world = [], [], []
    var = {0: [], 1: []}
    for b in range(2):
        order = list(range(V)) if b == 0 else list(reversed(range(V)))
        Kv, Ev = K[order].contiguous(), E[order].contiguous()
        pts_of = lambda dt: _world(dt, kinv, rinv, t, _COARSE_DEPTHS[b].to(dt).repeat_interleave(H * W), H, W)  # noqa: E731
        keys, fxy = _exact_taps(pts_of, Kv, Ev, H, W)
        if b == 0:
            assert torch.equal(keys, k_ref) and torch.equal(fxy, f_ref)
            _covers_the_edges(keys, fxy, V, H, W)
        p = torch.stack(pts_of(F64))
        assert torch.equal(p.float().double(), p)
        N = p.shape[1]
        tex = _texels(maps[b])
        f, fa = _sample(F64, tex, keys, fxy, H, W)
        var[0].append(_variance(f, fa))
        f1, fa1 = f.clone(), fa.clone()
        f1[0] = tex[0][torch.arange(N) % (H * W)]                      # view 0 contributes its un-warped map
        fa1[0] = f1[0].abs()
        var[1].append(_variance(f1, fa1))
        Kb.append(Kv)
        Eb.append(Ev)
        world.append(p)
    ref = {o: (torch.stack([x[0] for x in var[o]]), torch.stack([x[1] for x in var[o]])) for o in (0, 1)}
    cams = (kinv.repeat(2, 1), rinv.repeat(2, 1), t.repeat(2, 1), _COARSE_DEPTHS.clone(), torch.stack(Kb), torch.stack(Eb))
    return maps, cams, torch.stack(world), ref


@pytest.mark.parametrize("V", [1, 2, 3, 4, 5, 6, 7, 8])
def test_fetch_and_frustum_variance_exact_scene_every_view_count(dev, V):
    """pf_fetch_variance_f32 (ref_override 0 and 1, explicit points) and pf_frustum_variance_f32 (world points requested and
    world = NULL) at every V, B = 2, C = 3 (an odd count under the channel loop's unroll by two): against the float64
    variance with K_VAR(V); the world output equals the float64 points bit for bit."""
    H, W, C, B = _EH, _EW, 3, 2
    maps, (kinv, rinv, t, depths, K, E), world, ref = _coarse_reference(V)
    N = world.shape[2]
    d_maps = maps[:, :, :C].contiguous().to(dev)
    d_pts, d_K, d_E = world.float().contiguous().to(dev), K.to(dev), E.to(dev)
    worst = 0.0
    for override in (0, 1):
        out = _guarded(B * C * N, dev)
        _call("pf_fetch_variance_f32", _lib.ptr(d_maps), _lib.ptr(d_pts), _lib.ptr(d_K), _lib.ptr(d_E), _lib.ptr(out),
              B, V, C, H, W, N, override)
        got = _take(out, B * C * N, "fetch_variance").view(B, C, N).permute(0, 2, 1)
        worst = max(worst, _gate(got, ref[override][0][..., :C], ref[override][1][..., :C], K_VAR(V),
                                 "fetch_variance V%d override %d" % (V, override)))
    cams = [x.contiguous().to(dev) for x in (kinv, rinv, t, depths)]
    for want_world in (True, False):
        out = _guarded(B * C * N, dev)
        wbuf = _guarded(B * 3 * N, dev)
        _call("pf_frustum_variance_f32", _lib.ptr(d_maps), *([_lib.ptr(x) for x in cams] +
              [_lib.ptr(d_K), _lib.ptr(d_E), _lib.ptr(out), _lib.ptr(wbuf) if want_world else None, B, V, C, H, W, 3]))
        got = _take(out, B * C * N, "frustum_variance").view(B, C, N).permute(0, 2, 1)
        worst = max(worst, _gate(got, ref[1][0][..., :C], ref[1][1][..., :C], K_VAR(V),
                                 "frustum_variance V%d world %d" % (V, want_world)))
        w = wbuf.cpu()
        if want_world:
            assert torch.equal(_take(wbuf, B * 3 * N, "world").view(B, 3, N).double(), world)
        else:
            assert bool(torch.isnan(w[:B * 3 * N]).all())
    report("variance_planar_exact_V%d" % V, ratio_to_gate=worst, K=K_VAR(V))


@pytest.mark.parametrize("C", [4, 64, 68])
@pytest.mark.parametrize("V", [1, 2, 3, 4, 5, 6, 7, 8])
def test_frustum_variance_channel_last_exact_scene_every_view_count(dev, V, C):
    """pf_frustum_variance_cl_f32 against the same float64 reference with the same gate K_VAR(V) (its arithmetic is the
    planar kernel's): every V -- lane q projects view 1 + q % (V - 1) and the taps come by shuffle from lane v - 1 --,
    C = 4 (one live lane of 16), 64 (one full pass) and 68 (a second 64-channel pass with one live lane); N = 3 * 17 * 33 =
    1683 = 26 * 64 + 19, so the last block's shadow lanes run; B = 2; world requested and NULL."""
    H, W, B = _EH, _EW, 2
    maps, (kinv, rinv, t, depths, K, E), world, ref = _coarse_reference(V)
    N = world.shape[2]
    assert N % 64 != 0
    d_cl = maps[:, :, :C].permute(0, 1, 3, 4, 2).contiguous().to(dev)                       # (B, V, H, W, C)
    cams = [x.contiguous().to(dev) for x in (kinv, rinv, t, depths, K, E)]
    worst = 0.0
    for want_world in (True, False):
        out = _guarded(B * C * N, dev)
        wbuf = _guarded(B * 3 * N, dev)
        _call("pf_frustum_variance_cl_f32", _lib.ptr(d_cl), *([_lib.ptr(x) for x in cams] +
              [_lib.ptr(out), _lib.ptr(wbuf) if want_world else None, B, V, C, H, W, 3]))
        got = _take(out, B * C * N, "frustum_variance_cl").view(B, C, N).permute(0, 2, 1)
        worst = max(worst, _gate(got, ref[1][0][..., :C], ref[1][1][..., :C], K_VAR(V),
                                 "frustum_variance_cl V%d C%d world %d" % (V, C, want_world)))
        if want_world:
            assert torch.equal(_take(wbuf, B * 3 * N, "world").view(B, 3, N).double(), world)
        else:
            assert bool(torch.isnan(wbuf.cpu()[:B * 3 * N]).all())
    report("variance_cl_exact_V%d_C%d" % (V, C), ratio_to_gate=worst, K=K_VAR(V))


@pytest.mark.parametrize("S", [1, 63, 561])
@pytest.mark.parametrize("C", [4, 68, 130])
def test_nchw_to_nhwc_equals_permute(dev, C, S):
    """pf_nchw_to_nhwc_f32 (64 x 64 tiles through LDS) at channel counts and plane sizes that are no multiple of the tile,
    P = 2 planes: the bits of permute, nothing written behind the output."""
    g = torch.Generator().manual_seed(C * 1000 + S)
    x = torch.randn((2, C, S), generator=g)
    out, d_x = _guarded(2 * S * C, dev), x.to(dev)
    _call("pf_nchw_to_nhwc_f32", _lib.ptr(d_x), _lib.ptr(out), 2, C, S)
    got = _take(out, 2 * S * C, "nchw_to_nhwc").view(2, S, C)
    assert torch.equal(got, x.permute(0, 2, 1).contiguous())
    report("nchw_to_nhwc_C%d_S%d" % (C, S), mismatches=0.0)


def _flow_points(dt, kinv, rinv, t, depth, interval, H, W):
    """world points of the five hypotheses depth + interval (d - 2), n = d * H * W + y * W + x"""
    dop = depth.reshape(-1).to(dt).repeat(5) + interval.to(dt) * (torch.arange(5).repeat_interleave(H * W).to(dt) - 2.0)
    return _world(dt, kinv, rinv, t, dop, H, W)


def _flow_features_abi(dev, levels, widths, V, h, w, depth, interval, cam, ratio):
    """pf_flow_features_f32 into NaN-filled buffers with guard tails; an empty level gets a one-float placeholder (the
    entry point wants three pointers).  Returns feature (G * Ng, ctot), xyz (G, 3, Ng) on the CPU."""
    G, Ng = ratio * ratio, 5 * (h // ratio) * (w // ratio)
    ctot = sum(widths) + 24
    d_lv = [(torch.full((1,), NAN) if m is None else m).contiguous().to(dev) for m in levels]
    feat, xyz = _guarded(G * Ng * ctot, dev), _guarded(G * 3 * Ng, dev)
    d = [x.contiguous().to(dev) for x in (depth, interval, cam)]
    _call("pf_flow_features_f32", _lib.ptr(d_lv[0]), _lib.ptr(d_lv[1]), _lib.ptr(d_lv[2]), widths[0], widths[1], widths[2],
          V, h, w, _lib.ptr(d[0]), int(depth.shape[0]), int(depth.shape[1]), _lib.ptr(d[1]), _lib.ptr(d[2]), ratio,
          _lib.ptr(feat), _lib.ptr(xyz))
    f = _take(feat, G * Ng * ctot, "feature").view(G * Ng, ctot)
    x = _take(xyz, G * 3 * Ng, "xyz").view(G, 3, Ng)
    assert not bool(torch.isnan(f).any()) and not bool(torch.isnan(x).any()), "an element of feature / xyz was not written"
    return f, x


_CAM_MEAN = torch.tensor([3.5, -1.25, 520.0])            # dyadic
_CAM_STD = torch.tensor([64.0, 32.0, 128.0])             # powers of two: (world - mean) / std is exact in float32


@pytest.mark.parametrize("widths", [(16, 32, 64), (4, 0, 8), (36, 4, 68)])
@pytest.mark.parametrize("V", [1, 2, 3, 4, 5, 6, 7, 8])
def test_flow_features_exact_scene_every_view_count(dev, V, widths):
    """pf_flow_features_f32 at ratio 1 on the exact flow scene (prior 512, interval 64), every V, level widths with lanes
    masked by c < cl (4, 8, 36), an empty level, and chunks past 32 and 64 channels (36, 68); the 17 x 33 grid leaves the
    last row and column of 4 x 8 patches partly dead.  Variance columns: the float64 variance with K_VAR(V) (the sums start
    from 0: 0 + f is exact and fmaf(f, f, 0) is the one rounding of f * f).  xyz and the 24 repeated columns (column
    c1 + c2 + c3 + j holds axis j % 3): bit for bit -- mean dyadic, std a power of two, asserted exact on the CPU first.
    Every element is written, nothing beyond G * Ng * ctot is."""
    H, W = _EH, _EW
    (kinv, rinv, t, K, E, depth, interval), k64, f64 = _exact_reference(V, flow=True)
    _covers_the_edges(k64, f64, V, H, W)
    N = 5 * H * W
    cam = _cam_block(kinv, rinv, t, _CAM_STD, K, E)
    cam[21:24] = _CAM_MEAN
    xyz_of = lambda dt: ((torch.stack(_flow_points(dt, kinv, rinv, t, depth, interval, H, W)) - _CAM_MEAN.to(dt).view(3, 1))   # noqa: E731
                         / _CAM_STD.to(dt).view(3, 1))
    xyz64 = xyz_of(F64)
    assert torch.equal(xyz_of(F32).double(), xyz64)
    g = torch.Generator().manual_seed(4000 + 10 * V + widths[0])
    levels = [torch.randn((V, H, W, c), generator=g) if c else None for c in widths]
    csum = sum(widths)
    tex = torch.cat([m for m in levels if m is not None], dim=3).reshape(V, H * W, csum).double()
    f, fa = _sample(F64, tex, k64, f64, H, W)
    var, A = _variance(f, fa)
    feat, xyz = _flow_features_abi(dev, levels, widths, V, H, W, depth, interval, cam, 1)
    ratio = _gate(feat[:, :csum], var, A, K_VAR(V), "flow_features V%d %s" % (V, widths))
    assert torch.equal(xyz[0].double(), xyz64)
    for j in range(24):
        assert torch.equal(feat[:, csum + j].double(), xyz64[j % 3]), ("repeated xyz column", j)
    report("flow_features_exact_V%d_c%d_%d_%d" % ((V,) + tuple(widths)), ratio_to_gate=ratio, K=K_VAR(V))


# ---------------------------------------------------------------------------------------------
# 2. layout properties on generic cameras
# ---------------------------------------------------------------------------------------------
_GEN_WIDTHS = (8, 16, 4)


def _generic_inputs(dev, h, w, seed):
    """the tiny configuration's cameras (points of every view leave the map), a random three-level pyramid through
    pointflow.flow_pyramid (levels at (h, w), (h / 2, w / 2), (h / 4, w / 4)), a random prior"""
    kinv, rinv, t, K, E, V = _generic_scene()
    cam = _cam_block(kinv, rinv, t, torch.tensor([0.27, 1.31, 2.9]), K, E)
    cam[21:24] = torch.tensor([1.7, -0.6, 455.0])
    g = torch.Generator().manual_seed(seed)
    pyr = [torch.randn((V, c, h >> l, w >> l), generator=g) for l, c in enumerate(_GEN_WIDTHS)]
    levels = pointflow.flow_pyramid([p.to(dev) for p in pyr], h, w)
    torch.cuda.synchronize()
    assert torch.equal(levels[0].cpu(), pyr[0].permute(0, 2, 3, 1).contiguous())             # a level at (h, w) is transposed
    depth = 450.0 + 20.0 * torch.rand((h, w), generator=g)
    interval = torch.tensor([4.24 * 2.5 * 0.75])
    return levels, depth, interval, cam, V, g


def _features(levels, depth, interval, cam, h, w, ratio, dev):
    f, x = pointflow.flow_features(levels, depth.contiguous().to(dev), interval.to(dev), cam.to(dev), h, w, ratio)
    torch.cuda.synchronize()
    return f.cpu(), x.cpu()


@pytest.mark.parametrize("h,w", [(8, 12), (12, 20), (16, 24)])
def test_flow_features_sub_grid_order_equals_ratio_1_rows(dev, h, w):
    """feature[g, d hs ws + (y // r) ws + x // r] with g = (y % r) r + x % r equals row d h w + y w + x of the ratio-1
    call bit for bit, and likewise xyz, r in {2, 4} (through pointflow.flow_features)."""
    levels, depth, interval, cam, V, _ = _generic_inputs(dev, h, w, 5000 + h)
    f1, x1 = _features(levels, depth, interval, cam, h, w, 1, dev)
    d, y, x = torch.meshgrid(torch.arange(5), torch.arange(h), torch.arange(w), indexing="ij")
    row1 = (d * h * w + y * w + x).reshape(-1)
    for r in (2, 4):
        assert h % r == 0 and w % r == 0
        hs, ws = h // r, w // r
        fr, xr = _features(levels, depth, interval, cam, h, w, r, dev)
        gi = ((y % r) * r + x % r).reshape(-1)
        loc = (d * hs * ws + (y // r) * ws + x // r).reshape(-1)
        assert torch.equal(fr[gi, loc], f1[0, row1]), ("feature rows", h, w, r)
        assert torch.equal(xr[gi, :, loc], x1[0][:, row1].t()), ("xyz", h, w, r)
    report("flow_features_sub_grid_%dx%d" % (h, w), mismatches=0.0)


@pytest.mark.parametrize("h,w", [(8, 12), (12, 20), (16, 24)])
def test_flow_features_nearest_prior_equals_interpolated_prior(dev, h, w):
    """depth_in at (h, w), (h / 2, w / 2) and (5, 7) -- the last a non-integer upsampling -- gives the bits of the call on
    F.interpolate(depth, (h, w), mode="nearest") (evaluated on the CPU), at ratio 1 and 2."""
    levels, _, interval, cam, V, g = _generic_inputs(dev, h, w, 6000 + h)
    for dh, dw in ((h, w), (h // 2, w // 2), (5, 7)):
        small = 450.0 + 20.0 * torch.rand((dh, dw), generator=g)
        full = F.interpolate(small.view(1, 1, dh, dw), size=(h, w), mode="nearest")[0, 0].contiguous()
        for r in (1, 2):
            fa, xa = _features(levels, small, interval, cam, h, w, r, dev)
            fb, xb = _features(levels, full, interval, cam, h, w, r, dev)
            assert torch.equal(xa, xb), ("nearest source index differs from F.interpolate's", (dh, dw), (h, w), r)
            assert torch.equal(fa, fb), ("features", (dh, dw), (h, w), r)
    report("flow_features_nearest_%dx%d" % (h, w), mismatches=0.0)


def test_flow_features_rejects_before_launching(dev):
    """h % ratio != 0 -> PF_ERR_INVALID_ARG; V = 9 and c % 4 != 0 -> PF_ERR_UNSUPPORTED; the outputs keep their fill."""
    h, w, V = 8, 12, 3
    maps = torch.zeros((9, h, w, 8)).to(dev)
    depth, interval, cam = torch.full((h, w), 450.0).to(dev), torch.ones(1).to(dev), torch.zeros(27 + 21 * 9).to(dev)
    n = 9 * 5 * h * w * 48
    feat, xyz = torch.full((n,), SENT).to(dev), torch.full((n,), SENT).to(dev)

    def code(c1, c2, c3, V, h, w, ratio):
        return _raw("pf_flow_features_f32", _lib.ptr(maps), _lib.ptr(maps), _lib.ptr(maps), c1, c2, c3, V, h, w,
                    _lib.ptr(depth), 8, 12, _lib.ptr(interval), _lib.ptr(cam), ratio, _lib.ptr(feat), _lib.ptr(xyz))

    assert code(8, 8, 8, V, h, w, 3) == PF_ERR_INVALID_ARG           # 8 % 3
    assert code(8, 8, 8, V, h, w, 5) == PF_ERR_INVALID_ARG           # 8 % 5, 12 % 5
    assert code(8, 8, 8, 9, h, w, 2) == PF_ERR_UNSUPPORTED
    assert code(8, 6, 8, V, h, w, 2) == PF_ERR_UNSUPPORTED
    assert code(8, 8, 2, V, h, w, 1) == PF_ERR_UNSUPPORTED
    assert bool((feat.cpu() == SENT).all()) and bool((xyz.cpu() == SENT).all())
    assert _lib.status() == 0
    report("flow_features_rejections", launched=0.0)


def test_flow_features_generic_scene_values_away_from_integer_positions(dev):
    """One value check with rotations and non-dyadic intrinsics (ratio 1, 16 x 24, the tiny configuration's cameras).  The
    guard of test_gpu_warp_bwd._generic_check: only points whose float64 ix, iy in EVERY view lie further than delta = 10 x
    the float32 - float64 position drift (two torch evaluations of the formulas, measured on the CPU when the test runs)
    from an integer are compared -- there both sides read the same four texels -- and at most 1 % may be excluded
    (asserted on the float64 side alone).
    Gate: K_VAR(V) 2^-24 A + 2 delta Dmax * 4 M.  A position moved by up to delta in x and in y inside one cell moves the
    bilinear f by at most 2 delta Dmax, Dmax the largest difference of two neighbouring texels of the zero-padded maps (a
    border cell interpolates against 0).  The variance has d var / d f_v = (2 / V)(f_v - mean), so
    |d var| <= sum_v (2 / V) |f_v - mean| |d f_v| <= 2 * 2 M * max_v |d f_v| with M = max |texel| >= |f|: the Lipschitz
    factor of the variance in the max norm over views is 4 M.
    xyz: Kinv row (3), depth0 + interval (d - 2) (2), u * depth - t (2), Rinv row (3), - mean, / std (2): 12 -> K = 24."""
    h, w = 16, 24
    levels, depth, interval, cam, V, _ = _generic_inputs(dev, h, w, 7000)
    kinv, rinv, t, K, E, _ = _generic_scene()
    res = {dt: _project(dt, _flow_points(dt, kinv, rinv, t, depth, interval, h, w), K, E, h, w) for dt in (F32, F64)}
    k64, f64, ix64, iy64 = res[F64]
    drift = max(float((res[F32][2].double() - ix64).abs().max()), float((res[F32][3].double() - iy64).abs().max()))
    delta = 10.0 * drift
    far = (((ix64 - ix64.round()).abs() > delta) & ((iy64 - iy64.round()).abs() > delta)).all(dim=0)      # (N,)
    excluded = 1.0 - float(far.double().mean())
    assert excluded <= 0.01, excluded
    for v in range(1, V):
        assert bool((k64[v] != NOKEY).any()) and bool((k64[v] == NOKEY).any()), v
    lv = [m.cpu() for m in levels]
    csum = sum(_GEN_WIDTHS)
    tex = torch.cat(lv, dim=3).reshape(V, h * w, csum).double()
    f, fa = _sample(F64, tex, k64, f64, h, w)
    var, A = _variance(f, fa)
    padded = F.pad(torch.cat(lv, dim=3).double(), (0, 0, 1, 1, 1, 1))                          # (V, h + 2, w + 2, c)
    Dmax = max(float((padded[:, 1:] - padded[:, :-1]).abs().max()), float((padded[:, :, 1:] - padded[:, :, :-1]).abs().max()))
    M = float(tex.abs().max())
    feat, xyz = _features(levels, depth, interval, cam, h, w, 1, dev)
    err = (feat[0][:, :csum].double() - var).abs()
    bound = K_VAR(V) * U * A + 2.0 * delta * Dmax * 4.0 * M
    ratio = float((err / bound)[far].max())
    assert bool((err <= bound)[far].all()), ratio
    # xyz against float64 with every term's absolute value
    N = 5 * h * w
    pix = torch.arange(N) % (h * w)
    p = torch.stack([(pix % w).double() + 0.5, torch.div(pix, w, rounding_mode="floor").double() + 0.5, torch.ones(N, dtype=F64)])
    dabs = depth.reshape(-1).double().repeat(5) + 2.0 * float(interval)
    qa = (kinv.double().view(3, 3).abs() @ p) * dabs + t.double().abs().view(3, 1)
    mean, std = cam[21:24].double().view(3, 1), cam[24:27].double().view(3, 1)
    xa = (rinv.double().view(3, 3).abs() @ qa + mean.abs()) / std
    x64 = (torch.stack(_flow_points(F64, kinv, rinv, t, depth, interval, h, w)) - mean) / std
    rx = _gate(xyz[0], x64, xa, 24, "flow_features generic xyz")
    for j in range(24):
        assert torch.equal(feat[0][:, csum + j], xyz[0, j % 3])
    report("flow_features_generic_values", ratio_to_gate=ratio, K=K_VAR(V), position_drift_f32=drift, delta=delta,
           excluded_share=excluded, interpolation_allowance=2.0 * delta * Dmax * 4.0 * M, xyz_ratio_to_gate=rx, K_xyz=24)


# ---------------------------------------------------------------------------------------------
# 3. points the projection cannot place
# ---------------------------------------------------------------------------------------------
def test_fetch_points_the_projection_cannot_place(dev):
    """pf_fetch_forward_f32 and pf_fetch_variance_f32 (ref_override 0) with explicit points on the exact scene's first three
    views: behind the camera (the frustum points of plane 256 negated: they project like any other point), pz == 0 exactly
    (positions inf or NaN -- 0 / 0 for the view without translation --: every tap invalid, the view contributes 0), and |X|
    so large that ix leaves the int range (2^27 .. 3e38, where u itself overflows).  Finite maps; the output is finite
    everywhere, meets the float64 formula within the gates of section 1, and the status word stays 0."""
    H, W, V, C = _EH, _EW, 3, 2
    kinv, rinv, t, K, E = _exact_scene(V, flow=False)

    def pts_of(dt):
        X, Y, Z = _world(dt, kinv, rinv, t, torch.full((H * W,), 256.0, dtype=dt), H, W)
        behind = torch.stack([-X, -Y, -Z])
        zero = torch.tensor([[0.0, 1.0, -1.0, 40.0, -40.0, 0.0, 24.0, 3.0], [0.0, 0.0, 2.0, -8.0, 8.0, -32.0, 32.0, 1.0],
                             [0.0] * 8], dtype=dt)
        big = 2.0 ** 27
        far = torch.tensor([[big, -big, 1e30, -1e30, 3e38, -3e38, 1.0, 1e20], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -3e38, 1e20],
                            [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]], dtype=dt)
        return list(torch.cat([behind, zero, far], dim=1))

    keys, fxy = _exact_taps(pts_of, K, E, H, W, keyed_only=True)
    N = keys.shape[1]
    assert bool((keys[:, :H * W] != NOKEY).any())                    # points behind the camera land in the map
    assert bool((keys[:, H * W:] == NOKEY).all())                    # the others nowhere
    assert not bool(torch.isfinite(fxy[:, H * W:H * W + 8]).all())
    g = torch.Generator().manual_seed(8000)
    maps = torch.randn((1, V, C, H, W), generator=g)
    f, fa = _sample(F64, _texels(maps[0]), keys, fxy, H, W)
    assert bool(torch.isfinite(f).all()) and bool((f[:, H * W:] == 0).all())
    d_pts = torch.stack(pts_of(F32)).view(1, 3, N).contiguous().to(dev)
    d_maps, d_K, d_E = maps.to(dev), K.view(1, V, 9).to(dev), E.view(1, V, 12).to(dev)
    with torch.no_grad():                                            # (through the wrappers of utils.feature_fetcher)
        out = feature_fetcher.FeatureFetcher()(d_maps, d_pts, d_K.view(1, V, 3, 3), d_E.view(1, V, 3, 4))
        outv = feature_fetcher.fetch_variance(d_maps, d_pts, d_K.view(1, V, 3, 3), d_E.view(1, V, 3, 4))
    torch.cuda.synchronize()
    got = out.cpu().view(V, C, N).permute(0, 2, 1)
    r1 = _gate(got, f, fa, 14, "fetch_forward, unplaceable points")
    assert bool((got[:, H * W:] == 0).all())
    got = outv.cpu().view(C, N).t()
    var, A = _variance(f, fa)
    r2 = _gate(got, var, A, K_VAR(V), "fetch_variance, unplaceable points")
    assert bool((got[H * W:] == 0).all())
    assert _lib.status() == 0
    report("fetch_unplaceable_points", forward_ratio_to_gate=r1, K_forward=14, variance_ratio_to_gate=r2, K_variance=K_VAR(V))


# ---------------------------------------------------------------------------------------------
# 4. pf_flow_head_f32
# ---------------------------------------------------------------------------------------------
_HEAD_GRIDS = [(1, 1, 1), (3, 5, 1), (16, 16, 1), (16, 17, 1), (8, 12, 2), (8, 12, 4), (12, 12, 3)]
K_LOGIT_ROWS = 34        # explicit rows: fmaf(z, scale, shift) is one rounding of the exact value, then 16 fmaf: 17 -> 34
K_LOGIT_BN = 44          # resolved: invstd, invstd * gamma (2 on scale); (float)mean, its product with scale, beta - . (3, on
#                          top of scale's 2 inside the product: 5 on shift); the fmaf (1); 16 fmaf: 22 -> 44
K_SOFTMAX = 18           # expf to 1 ulp = 2 half-ulps in the numerator (2) and in the denominator's terms (2), the
#                          denominator's four additions (4), the division (1): 9 -> 18
K_DEPTH = 16             # (d - 2) * interval (1), its product with p (1), five additions into flow (5), depth + flow (1)
_EPS = float(torch.tensor(1e-5, dtype=F32))


def _head_sizes(h, w):
    sizes = [(h, w)]
    if h % 2 == 0 and w % 2 == 0:
        sizes.append((h // 2, w // 2))
    return sizes + [(5, 7)]


def _head_check(dev, name, h, w, ratio, ldz, dsize, Z, w_out, affine, K_logit, launch):
    """One launch of the head against float64.  Z (G, Ng, 16) float32 values; affine = (scale64, shift64, Pabs): rows
    (G, 16) the reference applies, Pabs None (A = sum |w| |a|: explicit rows, the fmaf rounds the exact value) or the
    absolute-value form of the shift (G, 16) (A = sum |w| (|z| |scale| + Pabs): the affine's own rounding is part of the
    path).  launch(Zbuf, depth_in, dh, dw, interval, flow_prob, depth_out) makes the call.
    Gates: logit K_logit u A;  p: softmax is 1/2-Lipschitz in the max norm (row d of its Jacobian is p_d (delta_dj - p_j),
    absolute row sum 2 p_d (1 - p_d) <= 1/2), its argument f_d - mx carries the logit error and the rounding of the
    subtraction (2 u |f_d - mx|), then K_SOFTMAX u p;  depth: sum_d |c_d| gate_p_d + K_DEPTH u (sum_d p_d |c_d| + |prior|)."""
    G, hs, ws = ratio * ratio, h // ratio, w // ratio
    Ng = 5 * hs * ws
    dh, dw = dsize
    Zbuf = torch.full((G * Ng, ldz), NAN)
    Zbuf[:, :16] = Z.reshape(G * Ng, 16)
    depth_in = (400.0 + 0.75 * torch.arange(dh * dw, dtype=F32)).view(dh, dw)                 # a ramp: every texel its own value
    interval = torch.tensor([2.65])
    prob, dout = _guarded(5 * h * w, dev), _guarded(h * w, dev)
    launch(Zbuf.to(dev), depth_in.to(dev), dh, dw, interval.to(dev), prob, dout)
    torch.cuda.synchronize()
    got_p = _take(prob, 5 * h * w, "flow_prob").view(5, h, w)
    got_d = _take(dout, h * w, "depth_out").view(h, w)
    scale, shift, Pabs = affine
    Z64, w64 = Z.double(), w_out.double()
    a = torch.relu(Z64 * scale.view(G, 1, 16) + shift.view(G, 1, 16))
    logit = (a * w64).sum(-1)                                                                  # (G, Ng)
    if Pabs is None:
        A = (a * w64.abs()).sum(-1)
    else:
        A = ((Z64.abs() * scale.abs().view(G, 1, 16) + Pabs.view(G, 1, 16)) * w64.abs()).sum(-1)
    d, y, x = torch.meshgrid(torch.arange(5), torch.arange(h), torch.arange(w), indexing="ij")
    gi, loc = (y % ratio) * ratio + x % ratio, d * hs * ws + (y // ratio) * ws + x // ratio
    fimg, Aimg = -logit[gi, loc], A[gi, loc]                                                   # (5, h, w), image order
    p = torch.softmax(fimg, dim=0)
    c = (torch.arange(5, dtype=F64) - 2.0).view(5, 1, 1) * float(interval)
    prior = F.interpolate(depth_in.view(1, 1, dh, dw), size=(h, w), mode="nearest")[0, 0].double()
    depth = prior + (p * c).sum(0)
    arg_err = K_logit * U * Aimg + 2.0 * U * (fimg - fimg.max(dim=0, keepdim=True)[0]).abs()
    gate_p = 0.5 * arg_err.max(dim=0, keepdim=True)[0] + K_SOFTMAX * U * p
    gate_d = (c.abs() * gate_p).sum(0) + K_DEPTH * U * ((p * c.abs()).sum(0) + prior.abs())
    assert bool(torch.isfinite(got_p).all()) and bool(torch.isfinite(got_d).all()), name
    rp = float(((got_p.double() - p).abs() / gate_p).max())
    rd = float(((got_d.double() - depth).abs() / gate_d).max())
    print("%s: prob %.4f of its gate, depth %.4f of its gate" % (name, rp, rd))
    assert rp <= 1.0 and rd <= 1.0, (name, rp, rd)
    return rp, rd, float(logit.abs().max())


def _head_values(h, w, ratio, seed, saturated):
    G, Ng = ratio * ratio, 5 * (h // ratio) * (w // ratio)
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn((G, Ng, 16), generator=g) + 0.3 * torch.randn((G, 1, 16), generator=g)    # every sub-grid its own rows
    w_out = 0.5 * torch.randn(16, generator=g) * (20.0 if saturated else 1.0)
    return Z, w_out, g


@pytest.mark.parametrize("saturated", [False, True])
@pytest.mark.parametrize("h,w,ratio", _HEAD_GRIDS)
def test_flow_head_explicit_rows_vs_float64(dev, h, w, ratio, saturated):
    """pf_flow_head_f32 with explicit (scale, shift) rows per sub-grid, ld_affine in {16, 24}, ldz in {16, 32} (NaN in the
    columns nobody may read), the prior at (h, w), (h / 2, w / 2) where that divides and (5, 7); one pixel, exactly one block,
    one pixel into a second block, ratios 2, 3, 4.  Each pixel is read from the sub-grid-major row and written in image order:
    Z differs per sub-grid and the prior is a ramp, so a transposed g, a wrong loc0 or a wrong nearest index leaves the gate.
    saturated: |logit| ~ 100 (the head sums its logits in float32, which the gate allows)."""
    G = ratio * ratio
    Z, w_out, g = _head_values(h, w, ratio, 9000 + 100 * h + w + ratio, saturated)
    worst_p = worst_d = top = 0.0
    for ldz in (16, 32):
        for dsize in _head_sizes(h, w):
            for ld in (16, 24):
                rows = torch.full((2, G, ld), NAN)
                rows[0, :, :16] = 1.0 + 0.3 * torch.randn((G, 16), generator=g)
                rows[1, :, :16] = 0.4 * torch.randn((G, 16), generator=g)
                d_rows, d_w = rows.to(dev), w_out.to(dev)

                def launch(Zb, dep, dh, dw, iv, prob, dout):
                    _call("pf_flow_head_f32", _lib.ptr(Zb), ldz, _lib.ptr(d_rows[0]), _lib.ptr(d_rows[1]), ld, None,
                          _lib.ptr(d_w), _lib.ptr(dep), dh, dw, _lib.ptr(iv), h, w, ratio, _lib.ptr(prob), _lib.ptr(dout))

                rp, rd, lg = _head_check(dev, "head rows %dx%d r%d ldz%d prior%s ld%d" % (h, w, ratio, ldz, dsize, ld), h, w,
                                         ratio, ldz, dsize, Z, w_out,
                                         (rows[0, :, :16].double(), rows[1, :, :16].double(), None), K_LOGIT_ROWS, launch)
                worst_p, worst_d, top = max(worst_p, rp), max(worst_d, rd), max(top, lg)
    if saturated and h * w > 1:
        assert top > 50.0, top
    report("flow_head_rows_%dx%d_r%d%s" % (h, w, ratio, "_saturated" if saturated else ""), prob_ratio_to_gate=worst_p,
           depth_ratio_to_gate=worst_d, K_logit=K_LOGIT_ROWS, K_softmax=K_SOFTMAX, K_depth=K_DEPTH, largest_logit=top)


def _head_bn_case(dev, h, w, ratio, T, ldz, dsize, seed, with_rows):
    """the head with a pending BatchNorm: statistics rows (G, T, pcols = 40, 2) float64 from a float64 split of Z's rows
    into T segments (empty ones where T exceeds the rows), the 16 channels at col0 = 8, NaN in every other column"""
    G, Ng = ratio * ratio, 5 * (h // ratio) * (w // ratio)
    Z, w_out, g = _head_values(h, w, ratio, seed, False)
    pcols, col0 = 40, 8
    Z64 = Z.double()
    partials = torch.full((G, T, pcols, 2), NAN, dtype=F64)
    cuts = [(Ng * i) // T for i in range(T + 1)]
    for i in range(T):
        seg = Z64[:, cuts[i]:cuts[i + 1]]
        partials[:, i, col0:col0 + 16, 0], partials[:, i, col0:col0 + 16, 1] = seg.sum(1), (seg * seg).sum(1)
    gamma = (1.0 + 0.3 * torch.randn(16, generator=g)).float()
    beta = (0.4 * torch.randn(16, generator=g)).float()
    mean = Z64.mean(1)                                                                         # (G, 16), float64 statistics
    var = (Z64 * Z64).mean(1) - mean * mean
    scale = gamma.double() / torch.sqrt(var + _EPS)
    shift = beta.double() - mean * scale
    Pabs = beta.double().abs() + (mean * scale).abs()
    ld = 24
    rows = torch.full((2, G, ld), NAN).to(dev)
    d_part, d_gamma, d_beta, d_w = partials.to(dev), gamma.to(dev), beta.to(dev), w_out.to(dev)
    job = _lib.BnJob(d_part.data_ptr(), T, pcols, col0, 16, float(Ng), float(Ng), d_gamma.data_ptr(), d_beta.data_ptr(),
                     None, None, 0.1, _EPS, G, 1, rows[0].data_ptr() if with_rows else None,
                     rows[1].data_ptr() if with_rows else None, ld if with_rows else 0, 0)

    def launch(Zb, dep, dh, dw, iv, prob, dout):
        _call("pf_flow_head_f32", _lib.ptr(Zb), ldz, None, None, 0, ctypes.pointer(job), _lib.ptr(d_w), _lib.ptr(dep), dh, dw,
              _lib.ptr(iv), h, w, ratio, _lib.ptr(prob), _lib.ptr(dout))

    res = _head_check(dev, "head in_bn %dx%d r%d T%d ldz%d prior%s" % (h, w, ratio, T, ldz, dsize), h, w, ratio, ldz, dsize, Z,
                      w_out, (scale, shift, Pabs), K_LOGIT_BN, launch)
    return res, rows.cpu(), (scale, shift, Pabs)


@pytest.mark.parametrize("h,w,ratio", _HEAD_GRIDS)
def test_flow_head_resolves_its_batchnorm_in_the_kernel(dev, h, w, ratio):
    """in_bn with G * 16 <= 256 and groups_per_stat == 1: every block reduces the statistics rows itself (the job carries no
    (scale, shift) rows: materialising them would be refused).  T in {1, 3, 40} partial rows, pcols = 40 > 16, col0 = 8;
    the reference's scale and shift come from the float64 statistics (the kernel's float64 sums over T rows differ from
    them by 1e-16 relative, nothing against 2^-24)."""
    assert ratio * ratio * 16 <= 256
    worst_p = worst_d = 0.0
    sizes = _head_sizes(h, w)
    i = 0
    for T in (1, 3, 40):
        for ldz in (16, 32):
            (rp, rd, _), _, _ = _head_bn_case(dev, h, w, ratio, T, ldz, sizes[i % len(sizes)], 9500 + 10 * h + w + T, False)
            worst_p, worst_d = max(worst_p, rp), max(worst_d, rd)
            i += 1
    report("flow_head_in_bn_%dx%d_r%d" % (h, w, ratio), prob_ratio_to_gate=worst_p, depth_ratio_to_gate=worst_d,
           K_logit=K_LOGIT_BN, K_softmax=K_SOFTMAX, K_depth=K_DEPTH)


def test_flow_head_materialises_the_rows_beyond_256_pairs(dev):
    """in_bn at ratio 5 on a (10, 10) grid: G * 16 = 400 > 256, the entry point writes the job's (scale, shift) rows with a
    finalize launch and the head reads them by sub-grid.  The rows themselves: scale carries 2 roundings (K = 4), shift 5
    against |beta| + |mean scale| (K = 10)."""
    worst_p = worst_d = 0.0
    for T, ldz, dsize in ((3, 16, (10, 10)), (40, 32, (5, 7)), (1, 32, (5, 5))):
        (rp, rd, _), rows, (scale, shift, Pabs) = _head_bn_case(dev, 10, 10, 5, T, ldz, dsize, 9900 + T, True)
        _gate(rows[0, :, :16], scale, scale.abs(), 4, "materialised scale rows")
        _gate(rows[1, :, :16], shift, Pabs, 10, "materialised shift rows")
        assert bool(torch.isnan(rows[:, :, 16:]).all())
        worst_p, worst_d = max(worst_p, rp), max(worst_d, rd)
    report("flow_head_in_bn_10x10_r5", prob_ratio_to_gate=worst_p, depth_ratio_to_gate=worst_d, K_logit=K_LOGIT_BN,
           K_softmax=K_SOFTMAX, K_depth=K_DEPTH)
