"""csrc/warp_bwd.hip kernel by kernel through the C ABI (as train_ops._warp_backward calls it; no autograd node on the tested
side), each entry point against a float64 evaluation of the formula its comment states.

The node tests (tests/test_gpu_train_ops.py: test_flow_feature_node_*, test_coarse_volume_node_*) project in float64 on the
reference side and therefore carry a 1e-4 gate (float32 tap positions, O(1) texel contrast).  Here the reference of the
value kernels (variance gradient, gather) takes the KEYS and FRACTIONAL OFFSETS the tested side uses as data -- synthetic
ones -- and never projects again: tap positions are identical on both sides and the gate is float32 rounding of the
arithmetic alone,
    |got - ref| <= K * 2^-24 * A,
A = the reference expression with every product and term replaced by its absolute value, K = twice the number of float32
roundings on the kernel's path (counted where each gate is built).  Every test reports its worst |got - ref| / (2^-24 A)
next to K.  The taps kernel itself is compared bit for bit on a scene whose projection is exact in float32, and on a generic
scene away from the integer positions where floor() is discontinuous.
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import report
from pointmvsnet_amd import _lib, synthetic, train_ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                       # unit roundoff of float32 (round to nearest)
NOKEY = 0xffffffff
F64 = torch.float64


def _call(name, *args):
    _lib.call(name, *(list(args) + [_lib.stream()]))
    torch.cuda.synchronize()


def _u32(keys):
    """int32 storage of uint32 keys -> int64 values"""
    return keys.cpu().to(torch.int64) & 0xffffffff


def _i32(keys64):
    """int64 values of uint32 keys -> int32 storage"""
    k = keys64.clone()
    k[k >= 2 ** 31] -= 2 ** 32
    return k.to(torch.int32)


# ---------------------------------------------------------------------------------------------
# the formulas of wb_world (warp_bwd.hip) and pf_project_taps (pf_common.h) in a dtype of choice
# ---------------------------------------------------------------------------------------------
def _world(dtype, kinv, rinv, t, depth_of_point, H, W):
    """world points of n = d * H * W + y * W + x; depth_of_point (N,) in `dtype`"""
    kinv, rinv, t = kinv.reshape(9).to(dtype), rinv.reshape(9).to(dtype), t.reshape(3).to(dtype)
    N = depth_of_point.numel()
    pix = torch.arange(N) % (H * W)
    px = (pix % W).to(dtype) + 0.5
    py = torch.div(pix, W, rounding_mode="floor").to(dtype) + 0.5
    u = [kinv[3 * i] * px + kinv[3 * i + 1] * py + kinv[3 * i + 2] for i in range(3)]
    q = [u[i] * depth_of_point - t[i] for i in range(3)]
    return [rinv[3 * i] * q[0] + rinv[3 * i + 1] * q[1] + rinv[3 * i + 2] * q[2] for i in range(3)]


def _project(dtype, xyz, K, E, H, W):
    """keys (V, N) int64, fxy (V, N, 2), ix, iy (V, N) of pf_project_taps + warp_taps_kernel's key, per view"""
    V = K.shape[0]
    K, E = K.reshape(V, 9).to(dtype), E.reshape(V, 12).to(dtype)
    X, Y, Z = xyz
    keys, fxy, ixs, iys = [], [], [], []
    cells = (H + 1) * (W + 1)
    for v in range(V):
        k, e = K[v], E[v]
        px = e[0] * X + e[1] * Y + e[2] * Z + e[3]
        py = e[4] * X + e[5] * Y + e[6] * Z + e[7]
        pz = e[8] * X + e[9] * Y + e[10] * Z + e[11]
        nx, ny = px / pz, py / pz
        uu = k[0] * nx + k[1] * ny + k[2]
        vv = k[3] * nx + k[4] * ny + k[5]
        gx = ((uu - 0.5) / (W - 1)) * 2.0 - 1.0
        gy = ((vv - 0.5) / (H - 1)) * 2.0 - 1.0
        ix = (gx + 1.0) * ((W - 1) / 2.0)
        iy = (gy + 1.0) * ((H - 1) / 2.0)
        x0, y0 = torch.floor(ix), torch.floor(iy)
        vx0, vx1 = (x0 >= 0) & (x0 <= W - 1), (x0 + 1 >= 0) & (x0 + 1 <= W - 1)
        vy0, vy1 = (y0 >= 0) & (y0 <= H - 1), (y0 + 1 >= 0) & (y0 + 1 <= H - 1)
        anyx, anyy = vx0 | vx1, vy0 | vy1
        xi = torch.where(anyx, x0, torch.zeros_like(x0)).to(torch.int64)
        yi = torch.where(anyy, y0, torch.zeros_like(y0)).to(torch.int64)
        key = v * cells + (yi + 1) * (W + 1) + (xi + 1)
        keys.append(torch.where(anyx & anyy, key, torch.full_like(key, NOKEY)))
        fxy.append(torch.stack([ix - x0, iy - y0], dim=1))
        ixs.append(ix)
        iys.append(iy)
    return torch.stack(keys), torch.stack(fxy), torch.stack(ixs), torch.stack(iys)


def _cam_block(kinv, rinv, t, std, K, E):
    """the packed PF_CAM_* block of include/pointflow_hip.h: Kref^-1, Rref^-1, tref, mean, std, then (K, E) per view"""
    V = K.shape[0]
    blk = torch.zeros(27 + 21 * V, dtype=torch.float32)
    blk[0:9], blk[9:18], blk[18:21] = kinv.reshape(9), rinv.reshape(9), t.reshape(3)
    blk[24:27] = std
    for v in range(V):
        blk[27 + 21 * v:36 + 21 * v] = K[v].reshape(9)
        blk[36 + 21 * v:48 + 21 * v] = E[v].reshape(12)
    return blk


def _taps_frustum(dev, kinv, rinv, t, depths, K, E, V, H, W, skip0):
    D = depths.numel()
    N = D * H * W
    keys = torch.full((V * N,), 7, dtype=torch.int32, device=dev)
    fxy = torch.full((V * N, 2), float("nan"), dtype=torch.float32, device=dev)
    a = [x.contiguous().to(dev) for x in (kinv, rinv, t, depths, K, E)]
    _call("pf_warp_taps_frustum_f32", *([_lib.ptr(x) for x in a] + [V, H, W, D, skip0, _lib.ptr(keys), _lib.ptr(fxy)]))
    return _u32(keys).view(V, N), fxy.cpu().view(V, N, 2)


def _taps_flow(dev, depth, interval, cam, V, H, W):
    N = 5 * H * W
    keys = torch.full((V * N,), 7, dtype=torch.int32, device=dev)
    fxy = torch.full((V * N, 2), float("nan"), dtype=torch.float32, device=dev)
    a = [x.contiguous().to(dev) for x in (depth, interval, cam)]
    _call("pf_warp_taps_flow_f32", *([_lib.ptr(x) for x in a] + [V, H, W, _lib.ptr(keys), _lib.ptr(fxy)]))
    return _u32(keys).view(V, N), fxy.cpu().view(V, N, 2)


# ---------------------------------------------------------------------------------------------
# (a) taps on a scene whose projection is exact in float32
# ---------------------------------------------------------------------------------------------
_EH, _EW = 17, 33                                  # H - 1 and W - 1 are powers of two: the grid normalisation divides exactly
# per-view (focal, cx, cy, tx, ty): identity rotations, power-of-two focals, dyadic principal points and translations.
# With the reference camera (16, 16.5, 8.5) a point of pixel x at depth z lands at ix = (f / 16) (x + .5 - 16.5) + f tx / z +
# cx - .5: view 0 on the texel centres (fx = fy = 0, the last column / row as cell W-1 / H-1), the others at dyadic
# fractions that change with the depth plane, into the cells xi = -1 / yi = -1, and out of the map.
_EXACT_VIEWS = [(16.0, 16.5, 8.5, 0.0, 0.0), (16.0, 16.5, 8.5, 40.0, -8.0), (16.0, 16.5, 8.5, -24.0, 32.0),
                (16.0, 16.5, 8.5, 640.0, 0.0), (32.0, 20.25, 8.5, -8.0, -8.0), (8.0, 16.5, 3.125, 0.0, 315.0),
                (16.0, 12.5, 8.5, 0.0, -1024.0), (16.0, 16.5, 8.5, -157.5, 78.75)]
# The flow stage's five hypotheses 512 + 64 (d - 2) = 64 * (6 .. 10) are not powers of two: t / z is dyadic for all five
# when t is a multiple of 315 / 4 = 78.75 (lcm(6 .. 10) = 2520 = 8 * 315).  (tx, ty) per view in units of 78.75.
_EXACT_FLOW_T = [(0, 0), (5, -1), (-3, 4), (80, 0), (-1, -1), (0, 4), (0, -128), (-2, 1)]


def _exact_scene(V, flow):
    kinv = torch.tensor([1 / 16.0, 0, -16.5 / 16.0, 0, 1 / 16.0, -8.5 / 16.0, 0, 0, 1.0])
    rinv, t = torch.eye(3).reshape(9), torch.zeros(3)
    K = torch.zeros(V, 9)
    E = torch.zeros(V, 12)
    for v, (f, cx, cy, tx, ty) in enumerate(_EXACT_VIEWS[:V]):
        if flow:
            tx, ty = 78.75 * _EXACT_FLOW_T[v][0], 78.75 * _EXACT_FLOW_T[v][1]
        K[v] = torch.tensor([f, 0, cx, 0, f, cy, 0, 0, 1.0])
        E[v] = torch.tensor([1.0, 0, 0, tx, 0, 1.0, 0, ty, 0, 0, 1.0, 0])
    return kinv, rinv, t, K, E


def _exact_reference(V, flow):
    kinv, rinv, t, K, E = _exact_scene(V, flow)
    H, W = _EH, _EW
    if flow:
        depth, interval = torch.full((H, W), 512.0), torch.tensor([64.0])
        dop = lambda dt: (depth.reshape(-1).to(dt).repeat(5)                                   # noqa: E731
                          + interval.to(dt) * (torch.arange(5).repeat_interleave(H * W).to(dt) - 2.0))
        extra = (depth, interval)
    else:
        depths = torch.tensor([256.0, 512.0, 1024.0])
        dop = lambda dt: depths.to(dt).repeat_interleave(H * W)                                 # noqa: E731
        extra = (depths,)
    out = {}
    for dt in (torch.float32, F64):
        out[dt] = _project(dt, _world(dt, kinv, rinv, t, dop(dt), H, W), K, E, H, W)
    k64, f64 = out[F64][0], out[F64][1]
    # the scene IS exact: a float32 evaluation of the same formulas gives the float64 keys and offsets bit for bit
    assert torch.equal(out[torch.float32][0], k64) and torch.equal(out[torch.float32][1].double(), f64)
    return (kinv, rinv, t, K, E) + extra, k64, f64


def _assert_exact_scene_covers_the_edges(keys, fxy, V, H, W):
    cells = (H + 1) * (W + 1)
    keyed = keys != NOKEY
    cell = torch.where(keyed, keys - torch.arange(V).view(V, 1) * cells, torch.zeros_like(keys))
    yi, xi = torch.div(cell, W + 1, rounding_mode="floor") - 1, cell % (W + 1) - 1
    assert bool((keyed & (fxy[..., 0] == 0) & (fxy[..., 1] == 0)).any())                      # on texel centres
    assert bool((keyed & (xi == W - 1)).any()) and bool((keyed & (yi == H - 1)).any())
    if V > 1:
        assert bool((~keyed).any())                                                           # fully outside
        assert bool((keyed & (xi == -1)).any()) and bool((keyed & (yi == -1)).any())
        inside = keyed & (xi >= 0) & (xi < W - 1) & (yi >= 0) & (yi < H - 1) & (fxy[..., 0] > 0) & (fxy[..., 1] > 0)
        assert bool(inside.any())


@pytest.mark.parametrize("V", [1, 3, 8])
def test_warp_taps_exact_scene_equals_the_formulas_bit_for_bit(dev, V):
    """pf_warp_taps_frustum_f32 (skip_view0 0 and 1) and pf_warp_taps_flow_f32 on cameras whose projection is exact in
    float32 (identity rotations, power-of-two focal lengths and depths / dyadic hypotheses, dyadic translations, a 17 x 33
    map): keys and fractional offsets equal a float64 evaluation of wb_world + pf_project_taps bit for bit.  The views put
    points strictly inside, on texel centres, into the border cells xi = -1, xi = W - 1, yi = -1, yi = H - 1, and outside."""
    H, W = _EH, _EW
    (kinv, rinv, t, K, E, depths), k64, f64 = _exact_reference(V, flow=False)
    _assert_exact_scene_covers_the_edges(k64, f64, V, H, W)
    for skip0 in (0, 1):
        keys, fxy = _taps_frustum(dev, kinv, rinv, t, depths, K, E, V, H, W, skip0)
        wk, wf = k64.clone(), f64.clone()
        if skip0:
            wk[0], wf[0] = NOKEY, 0.0
        assert torch.equal(keys, wk), ("frustum keys", skip0, int((keys != wk).sum()))
        assert torch.equal(fxy.double(), wf), ("frustum fxy", skip0)
    (kinv, rinv, t, K, E, depth, interval), k64, f64 = _exact_reference(V, flow=True)
    _assert_exact_scene_covers_the_edges(k64, f64, V, H, W)
    cam = _cam_block(kinv, rinv, t, torch.ones(3), K, E)
    keys, fxy = _taps_flow(dev, depth, interval, cam, V, H, W)
    assert torch.equal(keys, k64), ("flow keys", int((keys != k64).sum()))
    assert torch.equal(fxy.double(), f64), "flow fxy"
    report("warp_taps_exact_V%d" % V, mismatches=0.0)


# ---------------------------------------------------------------------------------------------
# (b) taps on the generic cameras of the tiny configuration
# ---------------------------------------------------------------------------------------------
def _generic_scene():
    """The cameras of synthetic.make_config("tiny") at the 16 x 24 coarse grid, the projecting intrinsics perturbed: every
    view's principal point moves by a few texels (so points of every view leave the map) and view 0's by a fraction (else
    the reference view projects its own pixel centres onto integers, where floor() is discontinuous)."""
    data, _, _ = synthetic.make_config("tiny", train_intrinsics=True)
    cams = data["cam_params_list"][0].double()                        # (V, 2, 4, 4): K of the 32 x 48 grid
    V = cams.shape[0]
    Kc = cams[:, 1, :3, :3].clone()
    Kc[:, :2, :] /= 2.0
    ext = cams[:, 0, :3, :4].clone()
    kinv = torch.inverse(Kc[0]).float()
    rinv = torch.inverse(ext[0, :, :3]).float()
    t = ext[0, :, 3].float()
    K = Kc.clone()
    for v in range(V):
        K[v, 0, 2] += (0.37, 5.3, -7.6)[v % 3]
        K[v, 1, 2] += (-0.41, -4.2, 6.1)[v % 3]
    return kinv, rinv, t, K.float().reshape(V, 9), ext.float().reshape(V, 12), V


def _generic_check(name, keys, fxy, r32, r64, skip0):
    k64, f64, ix64, iy64 = r64
    if skip0:
        keys, fxy, k64, f64, ix64, iy64 = keys[1:], fxy[1:], k64[1:], f64[1:], ix64[1:], iy64[1:]
        r32 = tuple(x[1:] for x in r32)
    drift = max(float((r32[2].double() - ix64).abs().max()), float((r32[3].double() - iy64).abs().max()))
    delta = 10.0 * drift
    far = ((ix64 - ix64.round()).abs() > delta) & ((iy64 - iy64.round()).abs() > delta)
    excluded = 1.0 - float(far.double().mean())
    keyed = far & (k64 != NOKEY)
    wrong = int((keys != k64)[far].sum())
    e_f = float((fxy.double() - f64).abs()[keyed].max())
    report(name, position_drift_f32=drift, delta=delta, excluded_share=excluded, wrong_keys=wrong, fxy_err=e_f,
           keyed_share=float(keyed.double().mean()))
    assert excluded <= 0.01, excluded
    for v in range(0 if skip0 else 1, k64.shape[0]):                  # every SOURCE view has points inside and outside the map
        assert bool((k64[v] != NOKEY).any()) and bool((k64[v] == NOKEY).any()), v
    assert wrong == 0 and e_f < delta, (wrong, e_f, delta)


def test_warp_taps_generic_scene_away_from_integer_positions(dev):
    """The taps kernels on the tiny configuration's cameras (rotations, non-dyadic intrinsics), points of every view
    leaving the map: keys equal the float64 keys wherever the float64 positions ix, iy are further than delta from an
    integer, and |fxy - fxy64| < delta there.  delta = 10 x the largest |ix32 - ix64| between a float32 and a float64
    TORCH evaluation of the formulas (not the kernel), measured on the CPU when the test runs.  Measured: frustum drift
    4.7e-06 -> delta 4.7e-05, 0.033 % of the pairs excluded; flow drift 5.2e-06 -> delta 5.2e-05, 0.017 % excluded
    (asserted <= 1 %, on the float64 side alone)."""
    kinv, rinv, t, K, E, V = _generic_scene()
    H, W = 16, 24
    depths = 425.0 + 10.6 * torch.arange(8, dtype=torch.float32)
    res = {dt: _project(dt, _world(dt, kinv, rinv, t, depths.to(dt).repeat_interleave(H * W), H, W), K, E, H, W)
           for dt in (torch.float32, F64)}
    keys, fxy = _taps_frustum(dev, kinv, rinv, t, depths, K, E, V, H, W, 1)
    assert bool((keys[0] == NOKEY).all()) and bool((fxy[0] == 0).all())
    _generic_check("warp_taps_generic_frustum", keys, fxy, res[torch.float32], res[F64], True)
    g = torch.Generator().manual_seed(71)
    depth = 450.0 + 20.0 * torch.rand((H, W), generator=g)
    interval = torch.tensor([4.24 * 2.5 * 0.75])
    cam = _cam_block(kinv, rinv, t, torch.ones(3), K, E)
    dop = lambda dt: (depth.reshape(-1).to(dt).repeat(5)                                       # noqa: E731
                      + interval.to(dt) * (torch.arange(5).repeat_interleave(H * W).to(dt) - 2.0))
    res = {dt: _project(dt, _world(dt, kinv, rinv, t, dop(dt), H, W), K, E, H, W) for dt in (torch.float32, F64)}
    keys, fxy = _taps_flow(dev, depth, interval, cam, V, H, W)
    _generic_check("warp_taps_generic_flow", keys, fxy, res[torch.float32], res[F64], False)


# ---------------------------------------------------------------------------------------------
# the taps of a pair from (key, fxy), float64 (wb_decode's statement, written independently)
# ---------------------------------------------------------------------------------------------
def _decode64(keys, fxy, H, W):
    """keys (V, N) int64, fxy (V, N, 2) -> texel offsets (4, V, N), weights (4, V, N) float64 (0 for a tap outside the map
    and for a pair without a key)"""
    V = keys.shape[0]
    cells = (H + 1) * (W + 1)
    keyed = keys != NOKEY
    cell = torch.where(keyed, keys - torch.arange(V).view(V, 1) * cells, torch.zeros_like(keys))
    assert bool(((cell >= 0) & (cell < cells)).all())
    yi, xi = torch.div(cell, W + 1, rounding_mode="floor") - 1, cell % (W + 1) - 1
    fx, fy = fxy[..., 0].double(), fxy[..., 1].double()
    offs, wgts = [], []
    for k in range(4):
        ty, tx = yi + (k >> 1), xi + (k & 1)
        ok = keyed & (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
        w = (fy if k >> 1 else 1.0 - fy) * (fx if k & 1 else 1.0 - fx)
        offs.append(torch.where(ok, ty * W + tx, torch.zeros_like(ty)))
        wgts.append(torch.where(ok, w, torch.zeros_like(w)))
    return torch.stack(offs), torch.stack(wgts)


def _synthetic_pairs(V, N, H, W, seed, nokey_share=0.1):
    """keys / fxy drawn directly: every cell yi in [-1, H-1], xi in [-1, W-1] (the border cells a quarter of a 9 x 13 map's),
    ~10 % pairs without a key, offsets in [0, 1) with exact 0 and 1 - 2^-24 among them"""
    g = torch.Generator().manual_seed(seed)
    cells = (H + 1) * (W + 1)
    cell = torch.randint(0, cells, (V, N), generator=g)
    cell[:, :4] = torch.tensor([0, W, H * (W + 1), cells - 1])        # the four corner cells
    keys = cell + torch.arange(V).view(V, 1) * cells
    keys[torch.rand((V, N), generator=g) < nokey_share] = NOKEY
    fxy = torch.rand((V, N, 2), generator=g)
    pick = torch.rand((V, N, 2), generator=g)
    fxy[pick < 0.1] = 0.0
    fxy[pick > 0.9] = 1.0 - 2.0 ** -24
    assert float(fxy.max()) < 1.0
    return keys, fxy.float()


# ---------------------------------------------------------------------------------------------
# (c) pf_variance_grad_f32
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [(4, 0, 0), (16, 32, 64), (8, 0, 4)])
@pytest.mark.parametrize("V", [1, 2, 3, 5, 8])
def test_variance_grad_vs_float64_from_the_same_taps(dev, V, levels):
    """gval[v][n][c] = (2 / V) dvar[n][c] (f_v - mean_v f), f_v the four-tap sum of view v's map from (key, fxy), against
    float64 on the same keys and offsets: every template instantiation V, one / three / two-of-three levels, dvar row-major
    (ldv = ctot, ldv = ctot + 24 with NaN in the unread columns) and channel-major, ref_override 0 and 1.
    Roundings on the path of one output: 1 - fx, 1 - fy, the weight product (3); the four taps (a product and three fmaf:
    4); the sum over views (V - 1); 1 / V, s * (1 / V), the difference, (2 / V) * g (2 / V itself is a scaling by two of
    1 / V's rounding, counted with it) and the last product (5): V + 11, taken as V + 12 -> K = 2 (V + 12)."""
    H, W, D = 9, 13, 27
    N = D * H * W                                                     # 3159 = 49 * 64 + 23
    ctot = sum(levels)
    g = torch.Generator().manual_seed(100 * V + ctot)
    keys, fxy = _synthetic_pairs(V, N, H, W, 100 * V + ctot + 1)
    maps = [torch.randn((V, H, W, c), generator=g) if c else None for c in levels]
    dvar = torch.randn((N, ctot), generator=g)
    off, wgt = _decode64(keys, fxy, H, W)
    cat = torch.cat([m for m in maps if m is not None], dim=3).double().view(V, H * W, ctot)
    K = 2 * (V + 12)
    d_keys, d_fxy = _i32(keys).reshape(-1).to(dev), fxy.reshape(-1, 2).contiguous().to(dev)
    d_maps = [None if m is None else m.to(dev) for m in maps]
    worst = 0.0
    for override in (0, 1):
        f = torch.zeros((V, N, ctot), dtype=F64)
        fa = torch.zeros((V, N, ctot), dtype=F64)
        for v in range(V):
            if v == 0 and override:
                f[v] = cat[0][torch.arange(N) % (H * W)]
                fa[v] = f[v].abs()
                continue
            for k in range(4):
                rows = cat[v][off[k, v]]
                f[v] += rows * wgt[k, v].view(N, 1)
                fa[v] += rows.abs() * wgt[k, v].view(N, 1)
        ref = (2.0 / V) * dvar.double() * (f - f.mean(dim=0, keepdim=True))
        A = (2.0 / V) * dvar.double().abs() * (fa + fa.mean(dim=0, keepdim=True))
        for layout in ("rows", "padded", "planar"):
            if layout == "rows":
                dv, ldv = dvar.clone(), ctot
            elif layout == "padded":
                dv, ldv = torch.full((N, ctot + 24), float("nan")), ctot + 24
                dv[:, :ctot] = dvar
            else:
                dv, ldv = dvar.t().contiguous(), -1
            d_dv = dv.to(dev)
            gval = torch.full((V, N, ctot), float("nan"), dtype=torch.float32, device=dev)
            _call("pf_variance_grad_f32", _lib.ptr(d_maps[0]), levels[0], _lib.ptr(d_maps[1]), levels[1],
                  _lib.ptr(d_maps[2]), levels[2], V, H, W, N, _lib.ptr(d_keys), _lib.ptr(d_fxy), _lib.ptr(d_dv), ldv,
                  override, _lib.ptr(gval))
            got = gval.cpu().double()
            assert bool(torch.isfinite(got).all()), (override, layout)
            err = (got - ref).abs()
            ratio = float((err / (U * A).clamp_min(1e-300))[A > 0].max())
            worst = max(worst, ratio)
            assert bool((err <= K * U * A).all()), (override, layout, ratio, K)
    report("variance_grad_V%d_c%d_%d_%d" % ((V,) + tuple(levels)), worst_over_u_A=worst, K=K, ratio_to_gate=worst / K)


# ---------------------------------------------------------------------------------------------
# (d) pf_sort_pairs_by_key + pf_warp_gather_f32
# ---------------------------------------------------------------------------------------------
def _gather_case(case, V, H, W):
    cells = (H + 1) * (W + 1)
    base = torch.arange(V).view(V, 1) * cells
    g = torch.Generator().manual_seed(len(case) + 17)
    if case == "spread":
        return _synthetic_pairs(V, 2999, H, W, 300)
    if case == "one_cell":                        # every pair of a view on ONE interior cell: a list beyond kSortCap = 1024
        N = 3001
        keys = base + torch.tensor([(3 + 1) * (W + 1) + (5 + 1), (6 + 1) * (W + 1) + (1 + 1), (3 + 1) * (W + 1) + (6 + 1)]
                                   )[:V].view(V, 1).expand(V, N)
    elif case == "tails":                         # list lengths 1 .. 17 on consecutive cells (the 8-per-trip tail)
        lens = torch.arange(1, 18)
        cell = (2 + 1) * (W + 1) + torch.repeat_interleave(torch.arange(17), lens)          # rows yi = 2 and 3, xi = -1 included
        N = int(lens.sum())
        perm = torch.stack([torch.randperm(N, generator=g) for _ in range(V)])               # point order is not cell order
        keys = base + cell[perm]
    elif case == "corners":
        N = 1501
        corner = torch.tensor([0, W, H * (W + 1), cells - 1])
        keys = base + corner[torch.randint(0, 4, (V, N), generator=g)]
    elif case == "empty_view":
        keys, fxy = _synthetic_pairs(V, 1999, H, W, 301)
        keys[1] = NOKEY
        return keys, fxy
    fxy = torch.rand(keys.shape + (2,), generator=g)
    fxy[:, ::5, 0] = 0.0
    fxy[:, 1::7, 1] = 1.0 - 2.0 ** -24
    return keys.contiguous(), fxy.float()


@pytest.mark.parametrize("case", ["spread", "one_cell", "tails", "corners", "empty_view"])
def test_sort_and_warp_gather_vs_dense_float64_accumulation(dev, case):
    """dmaps[v][texel] = sum over the pairs that tap the texel of weight * gval[pair], in list order, against a dense
    float64 index_add_ over (keys, fxy, gval); v0 in {0, 1, V} (v0 = V leaves dmaps untouched, views below v0 are never
    written, every texel of the others is), ctot in {4, 112}; two calls give equal bytes.
    Roundings per texel: 1 - fx, 1 - fy, the weight product (3) and one fmaf per list term -> K = 2 (terms + 4)."""
    V, H, W = 3, 9, 13
    keys, fxy = _gather_case(case, V, H, W)
    N = keys.shape[1]
    nkeys = V * (H + 1) * (W + 1)
    off, wgt = _decode64(keys, fxy, H, W)
    d_keys, d_fxy = _i32(keys).reshape(-1).to(dev), fxy.reshape(-1, 2).contiguous().to(dev)
    order, start = train_ops.sort_pairs(d_keys, nkeys)
    torch.cuda.synchronize()
    kept = keys.reshape(-1) < nkeys
    assert int(_u32(start)[-1]) == int(kept.sum())
    tex = (off + torch.arange(V).view(1, V, 1) * (H * W)).reshape(4, -1)                       # (4, V * N) rows of dmaps
    terms = torch.zeros(V * H * W, dtype=F64)
    for k in range(4):
        terms.index_add_(0, tex[k], (wgt[k].reshape(-1) != 0).double())
    PRE = 12345.678
    worst = 0.0
    for ctot in (4, 112):
        gen = torch.Generator().manual_seed(ctot)
        gval = torch.randn((V * N, ctot), generator=gen)
        ref = torch.zeros((V * H * W, ctot), dtype=F64)
        A = torch.zeros((V * H * W, ctot), dtype=F64)
        for k in range(4):
            ref.index_add_(0, tex[k], gval.double() * wgt[k].reshape(-1, 1))
            A.index_add_(0, tex[k], gval.double().abs() * wgt[k].reshape(-1, 1))
        ref, A = ref.view(V, H, W, ctot), A.view(V, H, W, ctot)
        Kt = (2.0 * (terms + 4.0)).view(V, H, W, 1)
        d_gval = gval.to(dev)
        for v0 in (0, 1, V):
            outs = []
            for _ in range(2):
                dmaps = torch.full((V, H, W, ctot), PRE, dtype=torch.float32, device=dev)
                _call("pf_warp_gather_f32", _lib.ptr(d_gval), _lib.ptr(d_fxy), _lib.ptr(order), _lib.ptr(start), V, v0, H, W,
                      ctot, _lib.ptr(dmaps))
                outs.append(dmaps.cpu())
            assert torch.equal(outs[0], outs[1])
            got = outs[0]
            assert bool((got[:v0] == PRE).all()), ("views below v0 written", v0)
            if v0 == V:
                continue
            assert bool((got[v0:] != PRE).all()), ("a texel kept its pre-fill value", v0)
            err = (got[v0:].double() - ref[v0:]).abs()
            bound = Kt[v0:] * U * A[v0:]
            pos = A[v0:] > 0
            if bool(pos.any()):
                worst = max(worst, float((err[pos] / bound[pos]).max()))
            assert bool((err <= bound).all()), (case, ctot, v0, float((err - bound).max()))
    report("warp_gather_%s" % case, ratio_to_gate=worst, longest_list_terms=float(terms.max()))


# ---------------------------------------------------------------------------------------------
# (e) pf_flow_depth_grad_f32
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (16, 24)])
def test_flow_depth_grad_vs_float64(dev, H, W):
    """d depth[y][x] = sum_d sum_axis (sum of the 8 repeats of dfeat[(d, y, x)][c0 + 3 r + axis]) *
    (Rinv Kinv (x + .5, y + .5, 1))[axis] / std[axis] against float64, c0 in {0, 5, 112} (5: rows not 16-byte aligned),
    ld in {c0 + 24, c0 + 29}, NaN in every column outside [c0, c0 + 24).
    Roundings: Kinv row (3), Rinv row (3), the division (1), the 8 repeats (8), the three axes (3), the five hypotheses (5):
    23 -> K = 46."""
    g = torch.Generator().manual_seed(H * W)
    kinv, rinv, t, K, E, V = _generic_scene()
    rinv = rinv + 0.05 * torch.randn((3, 3), generator=g)
    std = torch.tensor([0.27, 1.31, 2.9])
    cam = _cam_block(kinv, rinv, t, std, K, E).to(dev)
    pix = torch.arange(H * W)
    p = torch.stack([(pix % W).double() + 0.5, torch.div(pix, W, rounding_mode="floor").double() + 0.5,
                     torch.ones(H * W, dtype=F64)])                                          # (3, HW)
    u = kinv.double().view(3, 3) @ p
    ua = kinv.double().view(3, 3).abs() @ p
    dirs = (rinv.double().view(3, 3) @ u) / std.double().view(3, 1)                            # (3, HW)
    dira = (rinv.double().view(3, 3).abs() @ ua) / std.double().view(3, 1)
    Kc = 46
    worst = 0.0
    for c0 in (0, 5, 112):
        for ld in (c0 + 24, c0 + 29):
            dfeat = torch.full((5 * H * W, ld), float("nan"))
            vals = torch.randn((5 * H * W, 24), generator=g)
            dfeat[:, c0:c0 + 24] = vals
            v64 = vals.double().view(5, H * W, 8, 3)
            ref = (v64.sum(dim=2) * dirs.t().view(1, H * W, 3)).sum(dim=(0, 2))
            A = (v64.abs().sum(dim=2) * dira.t().view(1, H * W, 3)).sum(dim=(0, 2))
            d_dfeat = dfeat.to(dev)
            out = torch.full((H, W), float("nan"), dtype=torch.float32, device=dev)
            _call("pf_flow_depth_grad_f32", _lib.ptr(d_dfeat), ld, c0, _lib.ptr(cam), H, W, _lib.ptr(out))
            err = (out.cpu().double().view(-1) - ref).abs()
            worst = max(worst, float((err / (U * A)).max()))
            assert bool((err <= Kc * U * A).all()), (c0, ld, worst)
    report("flow_depth_grad_%dx%d" % (H, W), worst_over_u_A=worst, K=Kc, ratio_to_gate=worst / Kc)


# ---------------------------------------------------------------------------------------------
# (f) pf_resize_bilinear_backward_f32
# ---------------------------------------------------------------------------------------------
def _axis_envelope(in_size, out_size):
    """(in, out) 0/1 matrix: output index o interpolates from source index i -- |clamp(src, 0, in - 1) - i| < 1 -- with a
    margin of 1e-4 for the positions where a float32 and a float64 src fall on different sides of an integer"""
    src = (in_size / out_size) * (torch.arange(out_size, dtype=F64) + 0.5) - 0.5
    src = src.clamp(0.0, in_size - 1.0)
    return ((src.view(1, -1) - torch.arange(in_size, dtype=F64).view(-1, 1)).abs() < 1.0 + 1e-4).double()


def _resize_bwd(dev, dres, ld, c0, C, V, OH, OW, IH, IW):
    out = torch.full((V, C, IH, IW), float("nan"), dtype=torch.float32, device=dev)
    _call("pf_resize_bilinear_backward_f32", _lib.ptr(dres), ld, c0, C, V, OH, OW, IH, IW, _lib.ptr(out))
    return out.cpu()


@pytest.mark.parametrize("src,dst", [((5, 7), (5, 7)), ((8, 12), (4, 6)), ((16, 24), (4, 6)), ((4, 6), (8, 12)),
                                     ((4, 6), (16, 24)), ((4, 6), (32, 48)), ((7, 9), (20, 31)), ((20, 31), (7, 9)),
                                     ((1, 1), (4, 4)), ((4, 4), (1, 1)), ((3, 5), (3, 10))])
def test_resize_bilinear_backward_both_arms_vs_float64_autograd(dev, src, dst):
    """The adjoint of the bilinear resize (align_corners = False) of a pyramid level (V, C, IH, IW) -> (V, OH, OW, ld)
    columns [c0, c0 + C), against float64 autograd of F.interpolate: identity, / 2, / 4, x 2, x 4, x 8, non-integer ratios
    both ways, 1 x 1 on either side, one axis only; V in {1, 3}; the quad arm (C = 8, c0 in {0, 4}, ld % 4 == 0) and the
    scalar arm (C = 3; C = 4 with ld = 5; C = 4 with c0 = 2); NaN in every column outside [c0, c0 + C).  The two arms on the
    same values give the same bits.
    Gate: a source texel sums n = (rows in its window) x (columns in its window) terms g * wy * wx.  The kernel's positions
    src = fl(fl(IH / OH) * (o + .5)) - .5 carry three roundings of magnitude <= IH (IW) against the float64 reference, so a
    weight is off by up to (3 IH + 2) 2^-24 ABSOLUTE (l1 = src - i0, l0 = 1 - l1: 2 more) whatever its size; then the product
    wy * wx and one fmaf per term.  With A = the sum of |g| over the window (weights <= 1):
    |got - ref| <= (3 IH + 3 IW + 5 + n) 2^-24 A -> K = 2 (3 IH + 3 IW + 5 + n)."""
    (IH, IW), (OH, OW) = src, dst
    ey, ex = _axis_envelope(IH, OH), _axis_envelope(IW, OW)                                   # (IH, OH), (IW, OW)
    n_terms = ey.sum(dim=1).view(IH, 1) * ex.sum(dim=1).view(1, IW)
    Kt = 2.0 * (3 * IH + 3 * IW + 5 + n_terms)
    worst = 0.0
    for V in (1, 3):
        g = torch.Generator().manual_seed(IH * 1000 + OW + V)
        arms = [("quad", 8, 0, 8), ("quad", 8, 4, 12), ("scalar", 3, 0, 3), ("scalar", 4, 0, 5), ("scalar", 4, 2, 8)]
        for arm, C, c0, ld in arms:
            vals = torch.randn((V, OH, OW, C), generator=g)
            dres = torch.full((V, OH, OW, ld), float("nan"))
            dres[..., c0:c0 + C] = vals
            got = _resize_bwd(dev, dres.to(dev), ld, c0, C, V, OH, OW, IH, IW).double()
            x = torch.zeros((V, C, IH, IW), dtype=F64, requires_grad=True)
            gy = vals.double().permute(0, 3, 1, 2)
            F.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=False).backward(gy)
            A = torch.einsum("io,vcop,jp->vcij", ey, gy.abs(), ex)
            assert bool(torch.isfinite(got).all()), (arm, C, c0, ld)
            err = (got - x.grad).abs()
            bound = Kt.view(1, 1, IH, IW) * U * A
            pos = A > 0                                     # (a texel no output pixel reads: 0 on both sides, A = 0)
            worst = max(worst, float((err[pos] / bound[pos]).max()))
            assert bool((err <= bound).all()), (arm, V, C, c0, ld, worst)
        vals = torch.randn((V, OH, OW, 4), generator=g)
        quad = torch.full((V, OH, OW, 8), float("nan"))
        scal = torch.full((V, OH, OW, 5), float("nan"))
        quad[..., :4], scal[..., :4] = vals, vals
        a = _resize_bwd(dev, quad.to(dev), 8, 0, 4, V, OH, OW, IH, IW)
        b = _resize_bwd(dev, scal.to(dev), 5, 0, 4, V, OH, OW, IH, IW)
        assert torch.equal(a, b), "the quad and the scalar arm differ in bits"
    report("resize_bwd_%dx%d_to_%dx%d" % (IH, IW, OH, OW), ratio_to_gate=worst, largest_window_terms=float(n_terms.max()))
