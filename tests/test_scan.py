"""From predictions to the point cloud without files (pointmvsnet_amd/scan.py): ScanAccumulator and reconstruct_scan against
the file route -- eval_file_logger_host, probability_filter(NEAREST), load_pfm -- on a synthetic scan run through the real
model at the "tiny" configuration.  The three views of ``synthetic.make_config("tiny")`` take turns as the reference view."""
import os

import numpy as np
import pytest
import torch

from conftest import report
from pointmvsnet_amd import scan as S
from pointmvsnet_amd import synthetic
from pointmvsnet_amd.utils import eval_file_logger as EL
from pointmvsnet_amd.utils import io as IO

NAME = "flow2"
FUSE = {"disp_threshold": 50.0, "num_consistent": 1}         # untrained weights: loose enough for the cloud not to be empty


def _model(dev):
    from pointmvsnet_amd.model import PointMVSNet
    net = PointMVSNet()
    synthetic.seed_weights(net, seed=0)
    return net.to(dev).train()                               # the reference evaluates in train() mode (test.py:58)


def scan_batches(dev, paths=True):
    """One data_batch per view of the tiny scene as the reference view: (device batch, host batch)."""
    data, img_scales, inter_scales = synthetic.make_config("tiny", seed=3)
    V = data["img_list"].shape[1]
    g = torch.Generator().manual_seed(5)
    out = []
    for v in range(V):
        order = [v] + [u for u in range(V) if u != v]
        host = {"img_list": data["img_list"][:, order].contiguous(), "cam_params_list": data["cam_params_list"][:, order].contiguous(),
                "mean": data["mean"], "std": data["std"],
                "ref_img": torch.randint(0, 256, (1,) + tuple(data["img_list"].shape[3:]) + (3,), generator=g, dtype=torch.uint8)}
        batch = {k: t.to(dev) for k, t in host.items() if k != "ref_img"}
        batch["ref_img"] = host["ref_img"]
        batch["cam_params_list_host"] = host["cam_params_list"]
        batch["mean_host"], batch["std_host"] = host["mean"], host["std"]
        if paths:
            batch["ref_img_path"] = "/data/Eval/Rectified/scan4/rect_%03d_3_r5000.png" % (v + 1)
        out.append((batch, host))
    return out, img_scales, inter_scales


@pytest.fixture(scope="module")
def scan(dev):
    """The scan's batches and the model's predictions per view (cloned: the host copies of what the model returned)."""
    batches, img_scales, inter_scales = scan_batches(dev)
    net = _model(dev)
    preds = []
    with torch.no_grad():
        for batch, _ in batches:
            out = net(batch, img_scales, inter_scales, isFlow=True, isTest=True)
            preds.append({k: out[k].clone() for k in ("coarse_depth_map", "coarse_prob_map", "flow1", "flow1_prob", NAME,
                                                      NAME + "_prob")})
    return batches, preds, img_scales, inter_scales, net


def test_accumulator_refuses_what_it_cannot_do():
    with pytest.raises(ValueError):
        S.ScanAccumulator(3, mode="AREA")
    with pytest.raises(ValueError):
        S.ScanAccumulator(0)
    acc = S.ScanAccumulator(2)
    for call in (acc.filtered, acc.cameras, acc.fuse, acc.predictions):
        with pytest.raises(ValueError, match="have not been added"):
            call()
    preds = {"flow2": torch.zeros(1, 1, 4, 4), "flow2_prob": torch.zeros(1, 5, 4, 4), "coarse_prob_map": torch.zeros(1, 1, 2, 2)}
    batch = {"cam_params_list": torch.zeros(1, 1, 2, 4, 4), "img_list": torch.zeros(1, 1, 3, 16, 16)}
    with pytest.raises(RuntimeError, match="no CPU path"):
        acc.add(batch, preds, view_index=0)
    with pytest.raises(ValueError):
        acc.add(batch, preds, view_index=2)
    with pytest.raises(ValueError):
        acc.add(batch, {"flow2": preds["flow2"]}, view_index=0)


@pytest.mark.gpu
@pytest.mark.isolated
def test_accumulator_equals_the_stacked_predictions_and_the_file_route(dev, scan, tmp_path):
    batches, preds, _, _, _ = scan
    V = len(batches)
    acc = S.ScanAccumulator(V, name=NAME, mode="NEAREST")
    for (batch, _), p in zip(batches, preds):
        acc.add(batch, p)                                    # the view index comes from ref_img_path
    with pytest.raises(ValueError, match="added before"):
        acc.add(batches[0][0], preds[0])
    depths = torch.cat([p[NAME][:, 0] for p in preds])
    flow = torch.cat([p[NAME + "_prob"] for p in preds])
    init = torch.cat([p["coarse_prob_map"][:, 0] for p in preds])
    for a, b in zip(acc.predictions(), (depths, flow, init)):
        assert torch.equal(a, b)
    h, w = depths.shape[1:]
    assert init.shape[1:] == (h // 2, w // 2)
    want = S.filter_depth_maps(depths, flow, init, 0.2, 0.1, mode="NEAREST")
    got, kept = acc.filtered(return_kept=True)
    assert torch.equal(got, want) and kept.cpu().tolist() == [int((got[v] != 0).sum()) for v in range(V)]
    for mode in ("LANCZOS4", "CUBIC"):
        other = S.ScanAccumulator(V, name=NAME, mode=mode, init_prob_threshold=0.3, flow_prob_threshold=0.05)
        for v in (2, 0, 1):                                  # any order
            other.add(batches[v][0], preds[v], view_index=v)
        assert torch.equal(other.filtered(), S.filter_depth_maps(depths, flow, init, 0.3, 0.05, mode=mode))
    # the file route on the same predictions
    for v, ((_, host), p) in enumerate(zip(batches, preds)):
        EL.eval_file_logger_host(host, {k: t.cpu() for k, t in p.items()},
                                 str(tmp_path / "Eval" / "Rectified" / "scan4" / ("rect_%03d_3_r5000.png" % (v + 1))), "out")
    scene = str(tmp_path / "Eval" / "out" / "scan4")
    EL.probability_filter(scene, 0.2, 0.1, NAME, V, "NEAREST")
    files = np.stack([np.ascontiguousarray(IO.load_pfm(os.path.join(scene, "%08d_%s_prob_filtered.pfm" % (v, NAME)))[0])
                      for v in range(V)])
    assert files.tobytes() == got.cpu().numpy().tobytes()
    share = float((files != 0).mean())
    K, E = acc.cameras()
    assert K.dtype == np.float64 and K.shape == (V, 3, 3) and E.dtype == np.float64 and E.shape == (V, 4, 4)
    cams = [IO.load_cam_dtu(open(os.path.join(scene, "cam_%08d_%s.txt" % (v, NAME)))) for v in range(V)]
    assert np.allclose(np.stack([c[1, :3, :3] for c in cams]), K, rtol=1e-6, atol=0)
    assert np.allclose(np.stack([c[0] for c in cams]), E, rtol=1e-6, atol=1e-9)
    ref_h = batches[0][1]["img_list"].shape[3]
    for v in range(V):                                       # the intrinsics of the depth map's grid
        full = batches[v][1]["cam_params_list"][0, 0, 1, :3, :3].numpy()
        assert np.array_equal(K[v, 2], full[2]) and np.allclose(K[v, :2], full[:2] * (h / float(ref_h)), rtol=1e-7)
        assert np.array_equal(E[v], batches[v][1]["cam_params_list"][0, 0, 0].numpy().astype(np.float64))
    # the images: nearest-resized to the depth map, RGB
    images = acc.images()
    assert images.shape == (V, h, w, 3) and images.dtype == torch.uint8
    for v in range(V):
        ref = batches[v][1]["ref_img"][0].numpy()
        assert np.array_equal(images[v].cpu().numpy(), EL._resize_nearest(ref, h, w)[:, :, ::-1])
    # fused: the same bytes as fuse_depth_maps on the PFM-loaded depths and the accumulator's cameras
    from pointmvsnet_amd.fusion import fuse_depth_maps
    pts, col = acc.fuse(**FUSE)
    want_pts, want_col = fuse_depth_maps(torch.from_numpy(files).to(dev), K, E, images=images, **FUSE)
    assert pts.cpu().numpy().tobytes() == want_pts.cpu().numpy().tobytes()
    assert col.cpu().numpy().tobytes() == want_col.cpu().numpy().tobytes()
    out = str(tmp_path / "cloud.ply")
    acc.write_ply(out, **FUSE)
    back, back_col = IO.load_ply(out)
    assert np.array_equal(back, pts.cpu().numpy()) and np.array_equal(back_col, col.cpu().numpy())
    plain = S.ScanAccumulator(V, name=NAME, mode="NEAREST", keep_images=False)
    for (batch, _), p in zip(batches, preds):
        plain.add(batch, p)
    pts2, col2 = plain.fuse(**FUSE)
    assert col2 is None and plain.images() is None and torch.equal(pts2, pts)
    print("kept share", share, "points", int(pts.shape[0]))
    report("scan_accumulator", kept_share=share, points=int(pts.shape[0]))
    assert 0.0 < share <= 1.0 and pts.shape[0] > 0
    with pytest.raises(ValueError):                          # a view of another size
        bad = S.ScanAccumulator(V, name=NAME)
        bad.add(batches[0][0], preds[0])
        bad.add(batches[1][0], {k: t[..., :-1] for k, t in preds[1].items()})


@pytest.mark.gpu
def test_accumulated_views_survive_the_next_graph_replay(dev, scan):
    """GraphedForward returns STATIC buffers: what was added for view k must not change when view k + 1 is replayed."""
    if dev.type != "cuda":
        pytest.skip("hipGraph replay needs the hardware (tests/hipemu replays nothing)")
    from pointmvsnet_amd.graph import GraphedForward
    batches, preds, img_scales, inter_scales, _ = scan
    V = len(batches)
    acc = S.ScanAccumulator(V, name=NAME, mode="NEAREST")
    with torch.no_grad():
        g = GraphedForward(_model(dev), batches[0][0], img_scales, inter_scales, warmup=1)
        addresses = set()
        for v, (batch, _) in enumerate(batches):
            out = g(batch)
            addresses.add(out[NAME].data_ptr())
            acc.add(batch, out)                              # no synchronisation before the next replay
    assert len(addresses) == 1                               # the hazard is real: one buffer for every view
    torch.cuda.synchronize()
    depths, flow, init = acc.predictions()
    for v in range(V):                                       # replays equal eager bit for bit (tests/test_gpu_model.py)
        assert torch.equal(depths[v], preds[v][NAME][0, 0]), v
        assert torch.equal(flow[v], preds[v][NAME + "_prob"][0]) and torch.equal(init[v], preds[v]["coarse_prob_map"][0, 0])
    assert not torch.equal(depths[0], depths[1])


@pytest.mark.gpu
@pytest.mark.isolated
def test_reconstruct_scan_returns_the_accumulator_routes_points(dev, scan):
    batches, preds, img_scales, inter_scales, net = scan
    V = len(batches)
    acc = S.ScanAccumulator(V, name=NAME, mode="LANCZOS4")
    for (batch, _), p in zip(batches, preds):
        acc.add(batch, p)
    want, want_col = acc.fuse(**FUSE)
    pts, col, got = S.reconstruct_scan(net, (b for b, _ in batches), img_scales, inter_scales, view_num=V, name=NAME,
                                       fuse_kwargs=FUSE)
    assert isinstance(got, S.ScanAccumulator) and got.mode == "LANCZOS4"
    assert torch.equal(got.filtered(), acc.filtered())
    assert pts.cpu().numpy().tobytes() == want.cpu().numpy().tobytes() and torch.equal(col, want_col) and pts.shape[0] > 0
    # without paths the position in the iterable is the view index; a callable that is not a Module gets the batch alone
    nameless, _, _ = scan_batches(dev, paths=False)
    by_view = {id(b): p for (b, _), p in zip(nameless, preds)}
    pts2, _, _ = S.reconstruct_scan(lambda b: by_view[id(b)], [b for b, _ in nameless], name=NAME, fuse_kwargs=FUSE)
    assert torch.equal(pts2, pts)
    with pytest.raises(ValueError, match="have not been added"):
        S.reconstruct_scan(lambda b: by_view[id(b)], [b for b, _ in nameless][:2], view_num=V, name=NAME)
    with pytest.raises(ValueError):
        S.reconstruct_scan(lambda b: by_view[id(b)], [b for b, _ in nameless], name=NAME, mode="AREA")
