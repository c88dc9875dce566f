"""Reconstruct one DTU scan on the GPU, from the image folder to the point cloud (pointmvsnet_amd/scan.py): input and
preprocessing, the network, the batched confidence filter, the fusion and, optionally, the score -- no intermediate files.

    python tools/reconstruct_scan.py --root DTU --scan 9 --weights model.pth --out scan9.ply \
        [--mode LANCZOS4] [--init-prob-threshold 0.2] [--flow-prob-threshold 0.1] [--name flow2] \
        [--fusion roundtrip --num-src 10 --save-depth DIR] [--normals [--normal-step 2]] \
        [--voxel 0.2] [--outlier-radius 2.0 [--outlier-k 16] [--outlier-std 2.0] [--min-neighbors 4]] \
        [--mesh mesh.ply --mesh-voxel 0.5 [--mesh-trunc 2.0] [--mesh-min-weight 2] [--mesh-sparse] [--save-mesh-depth DIR]] \
        [--mesh-min-component 100] [--mesh-keep-largest 1] [--mesh-normals] [--mesh-sample-pitch 0.2] \
        [--mesh-simplify 2.0 [--mesh-simplify-placement mean]] \
        [--gt stl009_total.ply --obs-mask ObsMask9_10.mat --plane Plane9.mat [--depth-errors --splat 1]] \
        [--gt-mesh surface.ply --depth-errors] \
        [--photo-ncc 0.6 [--photo-radius 2 --photo-min-consistent 2 --photo-min-variance 25]] \
        [--upsample [--upsample-radius 2 --upsample-anchor-radius 1 --upsample-sigma-space 1.0 --upsample-sigma-colour 12.0
                     --upsample-rel-jump 0.02]] \
        [--speckle-size 100 --gap-size 7 [--segment-rel-jump 0.01]]

``--weights`` is a ``torch.load``-able file: its ``"model"`` entry if it has one, a leading ``module.`` stripped from the
keys.  ``--fusion roundtrip`` replaces the disparity fusion by the round-trip consistency filter
(pointmvsnet_amd/geometric.py) against the first ``--num-src`` views that ``Cameras/pair.txt`` lists for every view (0: all
other views); ``--save-depth DIR`` writes that filter's averaged depth map and mask of every view as ``%08d_geo.pfm`` and
``%08d_geo_mask.pfm``.  ``--normals`` writes the oriented cloud, ``x y z nx ny nz [red green blue]`` per vertex: normals from
the depth maps (pointmvsnet_amd/normals.py) with finite differences ``--normal-step`` pixels wide.  ``--voxel`` and
``--outlier-radius`` clean the fused cloud before it is written (pointmvsnet_amd/cloud_filter.py, ``clean_cloud``): a voxel
merge at that edge, then, inside that radius, the radius test with ``--min-neighbors`` (if given) and the statistical test
over ``--outlier-k`` neighbours at ``--outlier-std`` standard deviations (a negative value turns it off); colours and normals
are carried through.  Prints one JSON line: the
number of points, with ``--normals`` the number of them whose normal is undefined, the kept share per view, with cleaning its
``report`` (the point counts after each step) and, with ``--gt``,
the dict of ``evaluate_point_cloud`` -- with cleaning of the cleaned cloud, and of the cloud before it as ``score_before_cleaning``.  With ``--gt --depth-errors`` a second JSON line follows: the ground-truth cloud rendered
into every view (pointmvsnet_amd/render.py, ``--splat`` pixels around each projection) and ``depth_map_errors`` of the raw and of the
filtered depth maps against it, per view and in total, at thresholds of 1 and 3 times the reference view's depth interval
scaled for ``--name`` as ``PointMVSNetMetric`` scales it (coarse 1, flow1 0.75, flow2 0.375).
With ``--mesh`` the filtered depth maps are also integrated into a TSDF volume of pitch ``--mesh-voxel`` (truncation
``--mesh-trunc``, default 4 voxels) and its zero surface through the cells seen by ``--mesh-min-weight`` views is written as a PLY
with faces (pointmvsnet_amd/tsdf.py); the JSON line then carries ``mesh``: the grid size, the vertex and face counts and, with
``--gt``, ``evaluate_point_cloud`` of the mesh's vertices as ``score``, next to the cloud's.  ``--save-mesh-depth DIR`` also
rasterises that mesh back into the scan's own views (``ScanAccumulator.render_mesh``) and writes every view's fused,
hole-filled depth map as ``%08d_mesh.pfm``.  ``--mesh-sparse`` integrates into a sparse volume instead
(pointmvsnet_amd/sparse_tsdf.py: the same mesh, the state only near the surface, grids beyond 2^31 samples); ``mesh`` then
carries ``sparse``: the virtual and the allocated bricks and the state's bytes next to the dense volume's.
``--mesh-min-component N`` and ``--mesh-keep-largest K`` drop the mesh's connected components of fewer than ``N`` faces and
all but the ``K`` largest before it is written (pointmvsnet_amd/mesh_ops.py); ``mesh`` then carries the ``components``
report.  ``--mesh-normals`` writes area-weighted vertex normals, ``nx ny nz``, next to the faces.  With ``--gt``, ``mesh``
also gains ``score_sampled``: ``evaluate_point_cloud`` of ``sample_surface`` of the written mesh at ``--mesh-sample-pitch``
(default: the evaluation's ``min_dist``), next to the unchanged ``score`` of its vertices, whose density is the voxel's.
``--mesh-simplify CELL`` simplifies the mesh that is left (after the small components have gone, before the normals) by
vertex clustering on a grid of edge ``CELL`` with quadric placement (pointmvsnet_amd/mesh_simplify.py; ``mean`` with
``--mesh-simplify-placement``); ``mesh`` then carries ``simplify``: the report and the boundary / manifold / non-manifold edge
counts before and after, and with ``--gt`` also ``score_surface_before_simplification``.
With ``--gt-mesh FILE`` (a PLY with faces) ``--depth-errors`` scores against the rasterised surface instead of the splatted
cloud: no holes, and no back of the scene seen through a nearer surface; ``--splat`` is then not used.  The line's
``ground_truth`` names which of the two was used, ``"mesh"`` or ``"cloud"``.
With ``--mesh`` and ``--gt``, ``mesh`` also gains ``score_surface``: ``mesh_distance.evaluate_mesh`` of the written mesh, whose
completeness is the exact distance from every ground-truth point to the surface (pointmvsnet_amd/mesh_distance.py) and
whose accuracy uses the samples of ``score_sampled``; ``score`` and ``score_sampled`` are unchanged.  With ``--gt-mesh`` the first
line gains ``score_gt_mesh``: ``evaluate_point_cloud_on_mesh`` of the written cloud against that surface (``--obs-mask`` and
``--plane`` apply).
With ``--upsample`` the filtered depth maps are brought to the images' own grid before they are fused, guided by the images
(pointmvsnet_amd/refine.py; the image size must be an integer multiple of the depth map's, at most 8): the cloud that is
written, cleaned and scored is that of the upsampled maps, with colours from the full images.  The JSON line gains
``upsample``: the scale, the settings, ``points_low_grid`` and ``points_high_grid`` -- the fuser's cloud on either grid, before
any cleaning -- and, with ``--gt``, ``score_low_grid`` and ``score_high_grid`` of those two clouds.  ``--mesh``, ``--save-depth``
and ``--depth-errors`` keep working on the depth maps' own grid.
With ``--speckle-size N`` and / or ``--gap-size G`` the filtered depth maps are cleaned on their own grid before anything
consumes them (pointmvsnet_amd/depth_segments.py, ``clean_depth_maps``): segments of fewer than ``N`` pixels are removed, then
gaps of at most ``G`` pixels are interpolated over; two neighbours belong to one segment when their depths differ by at most
``--segment-rel-jump`` times the smaller.  The JSON line gains ``depth_cleaning``: the settings and the ``report`` of the
cleaning; with ``--gt`` also ``score_without_depth_cleaning``, ``evaluate_point_cloud`` of the cloud that the same fusion (and
cloud cleaning) gives without it; with ``--depth-errors`` the second line gains ``depth_errors_cleaned``, the errors of the
cleaned maps, next to ``depth_errors_filtered``, which stays those of the confidence filter's maps.
With ``--photo-ncc T`` the maps that are fused -- the upsampled ones under ``--upsample``, with the full images -- first pass the
photometric check (pointmvsnet_amd/photometric.py, ``photometric_filter``): a pixel stays when the windowed ZNCC of its
``2 R + 1`` window (``--photo-radius R``) reaches ``T`` in at least ``--photo-min-consistent`` of its ``--num-src`` source
views from ``pair.txt``; windows below ``--photo-min-variance`` are not scored and go.  The JSON line gains ``photometric``:
the settings and the filter's ``report`` (valid, scorable, kept and removed pixels per view and in total, also printed); with
``--gt`` also ``score_without_photometric``, ``evaluate_point_cloud`` of the cloud that the same fusion (and cloud cleaning)
gives without the check, next to ``score``.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_weights(model, path):
    import torch
    state = torch.load(path, map_location="cpu")
    if isinstance(state, dict) and "model" in state:
        state = state["model"]
    model.load_state_dict({(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()})


def batches_of(dataset, dev):
    """The dataset's items as the model's batches of one: a leading batch axis, device tensors, host copies of the cameras."""
    import torch
    for index in range(len(dataset)):
        item = dataset[index]
        batch = {"ref_img_path": item["ref_img_path"]}
        for key in ("img_list", "cam_params_list", "mean", "std", "ref_img"):
            batch[key] = torch.as_tensor(item[key])[None]
        batch["cam_params_list_host"] = batch["cam_params_list"]
        batch["mean_host"], batch["std_host"] = batch["mean"], batch["std"]
        for key in ("img_list", "cam_params_list", "mean", "std"):
            batch[key] = batch[key].to(dev)
        yield batch


INTERVAL_SCALE = {"coarse_depth_map": 1.0, "flow1": 0.75, "flow2": 0.375}      # PointMVSNetMetric's, per stage


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True, help="the DTU folder (Cameras/, Eval/Rectified/scan<N>/)")
    ap.add_argument("--scan", type=int, required=True)
    ap.add_argument("--out", required=True, help="the point cloud to write (binary PLY)")
    ap.add_argument("--weights", default=None, help="a torch.load-able state dict (default: seeded synthetic weights)")
    ap.add_argument("--mode", default="LANCZOS4", choices=["NEAREST", "BILINEAR", "CUBIC", "LANCZOS4"])
    ap.add_argument("--init-prob-threshold", type=float, default=0.2)
    ap.add_argument("--flow-prob-threshold", type=float, default=0.1)
    ap.add_argument("--disp-threshold", type=float, default=0.12)
    ap.add_argument("--num-consistent", type=int, default=3)
    ap.add_argument("--fusion", default="disparity", choices=["disparity", "roundtrip"])
    ap.add_argument("--num-src", type=int, default=10, help="roundtrip: source views per view from pair.txt (0: all others)")
    ap.add_argument("--pix-threshold", type=float, default=1.0)
    ap.add_argument("--rel-depth-threshold", type=float, default=0.01)
    ap.add_argument("--save-depth", default=None, help="folder for the round-trip filter's %%08d_geo.pfm / %%08d_geo_mask.pfm")
    ap.add_argument("--normals", action="store_true", help="write nx ny nz per vertex (normals from the depth maps)")
    ap.add_argument("--normal-step", type=int, default=1, help="--normals: the finite-difference baseline in pixels")
    ap.add_argument("--voxel", type=float, default=None, help="merge the fused points of every voxel of this edge")
    ap.add_argument("--outlier-radius", type=float, default=None, help="search radius of the outlier tests (none: no test)")
    ap.add_argument("--outlier-k", type=int, default=16, help="statistical test: neighbours per point")
    ap.add_argument("--outlier-std", type=float, default=2.0, help="statistical test: standard deviations kept (< 0: off)")
    ap.add_argument("--min-neighbors", type=int, default=None, help="radius test: neighbours needed inside --outlier-radius")
    ap.add_argument("--mesh", default=None, help="also write the scan as a triangle mesh (binary PLY with faces)")
    ap.add_argument("--mesh-voxel", type=float, default=0.5, help="--mesh: the pitch of the TSDF volume")
    ap.add_argument("--mesh-trunc", type=float, default=None, help="--mesh: the truncation distance (default: 4 voxels)")
    ap.add_argument("--mesh-min-weight", type=int, default=2, help="--mesh: views that must have seen every corner of a cell")
    ap.add_argument("--mesh-sparse", action="store_true",
                    help="--mesh: integrate into a sparse volume of 8 x 8 x 8 bricks (pointmvsnet_amd/sparse_tsdf.py)")
    ap.add_argument("--save-mesh-depth", default=None, help="--mesh: folder for every view's depth map of the mesh, %%08d_mesh.pfm")
    ap.add_argument("--mesh-min-component", type=int, default=None, help="--mesh: drop components of fewer faces")
    ap.add_argument("--mesh-keep-largest", type=int, default=None, help="--mesh: keep only this many components, the largest")
    ap.add_argument("--mesh-normals", action="store_true", help="--mesh: write area-weighted vertex normals")
    ap.add_argument("--mesh-simplify", type=float, default=None, metavar="CELL",
                    help="--mesh: simplify the mesh by vertex clustering on a grid of this edge (pointmvsnet_amd/mesh_simplify.py)")
    ap.add_argument("--mesh-simplify-placement", default="quadric", choices=["quadric", "mean"],
                    help="--mesh-simplify: where a cluster's vertex goes")
    ap.add_argument("--mesh-sample-pitch", type=float, default=None,
                    help="--mesh with --gt: the pitch of the surface samples that are scored (default: the evaluation's min_dist)")
    ap.add_argument("--name", default="flow2")
    ap.add_argument("--num-view", type=int, default=5)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--num-virtual-plane", type=int, default=96)
    ap.add_argument("--interval-scale", type=float, default=2.13)
    ap.add_argument("--img-scales", type=float, nargs="+", default=[0.125, 0.25, 0.5])
    ap.add_argument("--inter-scales", type=float, nargs="+", default=[1.0, 0.75, 0.15])
    ap.add_argument("--lighting", type=int, default=3)
    ap.add_argument("--gt", default=None, help="the scan's ground-truth cloud (PLY): score the result")
    ap.add_argument("--obs-mask", default=None, help="DTU's ObsMask<scan>_10.mat")
    ap.add_argument("--plane", default=None, help="DTU's Plane<scan>.mat")
    ap.add_argument("--gt-mesh", default=None, help="the scan's ground-truth surface (PLY with faces) for --depth-errors")
    ap.add_argument("--depth-errors", action="store_true", help="with --gt or --gt-mesh: one more JSON line of per-view depth errors")
    ap.add_argument("--splat", type=int, default=1, help="--depth-errors: pixels around a projection that a point fills")
    ap.add_argument("--upsample", action="store_true", help="fuse the depth maps upsampled to the images' grid, guided by the images")
    ap.add_argument("--upsample-radius", type=int, default=2, help="--upsample: taps out to this many low-resolution pixels")
    ap.add_argument("--upsample-anchor-radius", type=int, default=1, help="--upsample: the anchor's window (0: nearest replication's edges)")
    ap.add_argument("--upsample-sigma-space", type=float, default=1.0, help="--upsample: in low-resolution pixels")
    ap.add_argument("--upsample-sigma-colour", type=float, default=12.0, help="--upsample: in mean absolute channel difference")
    ap.add_argument("--upsample-rel-jump", type=float, default=0.02, help="--upsample: relative depth jump that a tap may not bridge")
    ap.add_argument("--speckle-size", type=int, default=None, help="remove depth-map segments of fewer pixels than this")
    ap.add_argument("--gap-size", type=int, default=None, help="interpolate over depth-map gaps of at most this many pixels (<= 32)")
    ap.add_argument("--segment-rel-jump", type=float, default=0.01,
                    help="--speckle-size, --gap-size: neighbours are linked up to this relative depth difference")
    ap.add_argument("--photo-ncc", type=float, default=None,
                    help="photometric check before the fusion: a source agrees at a windowed ZNCC of at least this")
    ap.add_argument("--photo-radius", type=int, default=2, help="--photo-ncc: the window is 2 R + 1 pixels wide (1..5)")
    ap.add_argument("--photo-min-consistent", type=int, default=2, help="--photo-ncc: agreeing sources a pixel needs")
    ap.add_argument("--photo-min-variance", type=float, default=25.0,
                    help="--photo-ncc: least grey-level variance of a window that is scored")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if args.save_mesh_depth and not args.mesh:
        ap.error("--save-mesh-depth needs --mesh")
    import torch
    from pointmvsnet_amd import cloud_filter, evaluation, geometric, scan, synthetic
    from pointmvsnet_amd.dataset import DTUDataset
    from pointmvsnet_amd.model import PointMVSNet
    from pointmvsnet_amd.utils import io
    dev = torch.device(args.device)
    net = PointMVSNet()
    if args.weights:
        load_weights(net, args.weights)
    else:
        synthetic.seed_weights(net, seed=0)
    net = net.to(dev).train()                                # the reference evaluates in train() mode (test.py:58)
    dataset = DTUDataset(args.root, "test", num_view=args.num_view, height=args.height, width=args.width,
                         num_virtual_plane=args.num_virtual_plane, interval_scale=args.interval_scale, device=dev,
                         scans=[args.scan], lightings=[args.lighting])
    sources = geometric.sources_from_pairs(dataset.cluster_list, len(dataset), args.num_src) if args.num_src > 0 else None
    geo_kwargs = {"sources": sources, "pix_threshold": args.pix_threshold, "rel_depth_threshold": args.rel_depth_threshold,
                  "num_consistent": args.num_consistent}
    fuse_kwargs = {"disp_threshold": args.disp_threshold, "num_consistent": args.num_consistent}
    if args.fusion == "roundtrip":
        fuse_kwargs = dict(geo_kwargs, method="roundtrip")
    if args.normals:
        fuse_kwargs.update(with_normals=True, normal_step=args.normal_step)
    photo = None
    if args.photo_ncc is not None:
        photo = {"sources": sources, "radius": args.photo_radius, "min_variance": args.photo_min_variance,
                 "ncc_threshold": args.photo_ncc, "num_consistent": args.photo_min_consistent}
        fuse_kwargs["photo"] = photo
    low_grid_kwargs = dict(fuse_kwargs)
    upsample = None
    if args.upsample:
        upsample = {"radius": args.upsample_radius, "anchor_radius": args.upsample_anchor_radius,
                    "sigma_space": args.upsample_sigma_space, "sigma_colour": args.upsample_sigma_colour,
                    "rel_jump": args.upsample_rel_jump}
        fuse_kwargs["upsample"] = upsample
    clean_depth = None
    if args.speckle_size is not None or args.gap_size is not None:
        clean_depth = {"min_size": args.speckle_size or 0, "max_gap": args.gap_size or 0, "rel_jump": args.segment_rel_jump}
    points, colours, *normals, acc = scan.reconstruct_scan(
        net, batches_of(dataset, dev), tuple(args.img_scales), tuple(args.inter_scales), view_num=len(dataset),
        fuse_kwargs=fuse_kwargs, name=args.name, keep_guides=args.upsample, clean_depth=clean_depth,
        mode=args.mode, init_prob_threshold=args.init_prob_threshold, flow_prob_threshold=args.flow_prob_threshold)
    normals = normals[0] if normals else None
    clean = {}
    if args.voxel is not None:
        clean["voxel"] = args.voxel
    if args.outlier_radius is not None:
        clean.update(max_radius=args.outlier_radius, k=args.outlier_k, min_neighbors=args.min_neighbors,
                     std_ratio=args.outlier_std if args.outlier_std >= 0 else None)
    elif args.min_neighbors is not None:
        ap.error("--min-neighbors needs --outlier-radius")
    raw_points = points
    if clean:                                                # what ScanAccumulator.fuse(clean=...) does; here both clouds are kept
        points, colours, normals, report = cloud_filter.clean_cloud(points, colours, normals, **clean)
    io.write_ply(args.out, points.cpu().numpy(), None if colours is None else colours.cpu().numpy(),
                 None if normals is None else normals.cpu().numpy())
    filtered, kept = acc.filtered(return_kept=True)
    out = {"scan": args.scan, "views": len(dataset), "mode": args.mode, "fusion": args.fusion, "points": int(points.shape[0]), "out": args.out,
           "kept_share_per_view": [k / float(filtered[0].numel()) for k in kept.cpu().tolist()]}
    if clean_depth is not None:
        out["depth_cleaning"] = dict(clean_depth, report=acc.last_depth_report)
    if photo is not None:
        out["photometric"] = dict({k: v for k, v in photo.items() if k != "sources"}, num_src=args.num_src,
                                  report=acc.last_photo_report)
        print("photometric: %(valid)d valid pixels, %(scorable)d scorable, %(kept)d kept, %(removed)d removed"
              % acc.last_photo_report["total"], file=sys.stderr)
    low_grid_points = None
    if upsample is not None:
        low_grid_points = acc.fuse(**low_grid_kwargs)[0]
        out["upsample"] = dict(upsample, scale=int(acc.guides().shape[1]) // int(filtered.shape[1]),
                               points_low_grid=int(low_grid_points.shape[0]), points_high_grid=int(raw_points.shape[0]))
    if clean:
        out["report"] = report
    if normals is not None:
        out["normals_undefined"] = int((normals == 0).all(dim=1).sum())
    mesh_vertices = None
    if args.mesh:
        from pointmvsnet_amd import tsdf
        mesh_kwargs = {"voxel": args.mesh_voxel, "trunc": args.mesh_trunc, "min_weight": args.mesh_min_weight}
        mesh_trunc = 4.0 * args.mesh_voxel if args.mesh_trunc is None else args.mesh_trunc
        K, E = acc.cameras()
        _, dims = tsdf.dims_for(tsdf.volume_bounds(filtered, K, E, pad=mesh_trunc), args.mesh_voxel,   # the grid mesh() builds
                                max_samples=2 ** 60 - 1 if args.mesh_sparse else None)
        if args.mesh_sparse:
            mesh_kwargs.update(sparse=True)
        if args.mesh_min_component is not None or args.mesh_keep_largest is not None:
            mesh_kwargs.update(min_component_faces=args.mesh_min_component, keep_largest=args.mesh_keep_largest)
        if args.mesh_normals:
            mesh_kwargs.update(with_normals=True)
        unsimplified = None
        if args.mesh_simplify is not None:                       # one integration: the mesh as extracted, then its simplification
            from pointmvsnet_amd import mesh_ops, mesh_simplify
            mesh_simplify.check_simplify_arguments("--mesh-simplify", args.mesh_simplify, args.mesh_simplify_placement)
            unsimplified = acc.mesh(**dict(mesh_kwargs, with_normals=False))
            mesh_vertices, faces, mesh_colours, simplify_report = mesh_simplify.simplify_mesh(
                unsimplified[0], unsimplified[1], args.mesh_simplify, colours=unsimplified[2],
                placement=args.mesh_simplify_placement)
            mesh_normals = mesh_ops.vertex_normals(mesh_vertices, faces) if args.mesh_normals else None
            io.write_ply(args.mesh, mesh_vertices.cpu().numpy(), None if mesh_colours is None else mesh_colours.cpu().numpy(),
                         None if mesh_normals is None else mesh_normals.cpu().numpy(), faces=faces.cpu().numpy())
        else:
            mesh_vertices, faces = acc.write_mesh(args.mesh, **mesh_kwargs)[:2]
        out["mesh"] = {"out": args.mesh, "voxel": args.mesh_voxel, "trunc": mesh_trunc, "min_weight": args.mesh_min_weight,
                       "dims": list(dims), "vertices": int(mesh_vertices.shape[0]), "faces": int(faces.shape[0])}
        if acc.last_mesh_report is not None:
            out["mesh"]["components"] = acc.last_mesh_report
        if acc.last_sparse_report is not None:
            out["mesh"]["sparse"] = acc.last_sparse_report
        if unsimplified is not None:
            out["mesh"]["simplify"] = dict(simplify_report, cell=args.mesh_simplify, placement=args.mesh_simplify_placement,
                                           edges_before=mesh_simplify.mesh_edge_counts(unsimplified[1]),
                                           edges_after=mesh_simplify.mesh_edge_counts(faces))
            print("simplified at cell %g (%s): %s" % (args.mesh_simplify, args.mesh_simplify_placement,
                                                      json.dumps(out["mesh"]["simplify"])), file=sys.stderr)
        print("mesh: grid %d x %d x %d, %d vertices, %d faces" % (tuple(dims) + (out["mesh"]["vertices"], out["mesh"]["faces"])),
              file=sys.stderr)
        if args.save_mesh_depth:
            os.makedirs(args.save_mesh_depth, exist_ok=True)
            mesh_depth = acc.render_mesh(mesh_vertices, faces).cpu().numpy()
            for v in range(len(dataset)):
                io.write_pfm(os.path.join(args.save_mesh_depth, "%08d_mesh.pfm" % v), mesh_depth[v])
            out["mesh"]["filled_share_per_view"] = [float((d > 0).mean()) for d in mesh_depth]
    if args.save_depth:
        import numpy as np
        os.makedirs(args.save_depth, exist_ok=True)
        depth_avg, mask, _ = acc.geometric(return_points=False, **geo_kwargs)
        depth_avg, mask = depth_avg.cpu().numpy(), mask.cpu().numpy().astype(np.float32)
        for v in range(len(dataset)):
            io.write_pfm(os.path.join(args.save_depth, "%08d_geo.pfm" % v), depth_avg[v])
            io.write_pfm(os.path.join(args.save_depth, "%08d_geo_mask.pfm" % v), mask[v])
        out["kept_share_per_view_geo"] = [float(m.mean()) for m in mask]
    if args.gt:
        kw = {}
        if args.obs_mask:
            mask, bb_min, res = io.load_dtu_obs_mask(args.obs_mask)
            kw.update(obs_mask=torch.from_numpy(mask), bb_min=bb_min, res=res)
        if args.plane:
            kw.update(plane=io.load_dtu_plane(args.plane))
        gt = torch.from_numpy(io.load_ply_points(args.gt)).to(dev)
        out["score"] = evaluation.evaluate_point_cloud(points, gt, **kw)
        if clean:
            out["score_before_cleaning"] = evaluation.evaluate_point_cloud(raw_points, gt, **kw)
        if clean_depth is not None:                          # the same fusion and cloud cleaning of the maps as the filter left them
            acc.clean_depth = None
            uncleaned = acc.fuse(**fuse_kwargs)
            acc.clean_depth = clean_depth
            if clean:
                uncleaned = cloud_filter.clean_cloud(uncleaned[0], uncleaned[1], None, **clean)
            out["score_without_depth_cleaning"] = evaluation.evaluate_point_cloud(uncleaned[0], gt, **kw)
        if photo is not None:                                # the same fusion and cloud cleaning without the photometric check
            unchecked = acc.fuse(**{k: v for k, v in fuse_kwargs.items() if k != "photo"})
            if clean:
                unchecked = cloud_filter.clean_cloud(unchecked[0], unchecked[1], None, **clean)
            out["photometric"]["points_without"] = int(unchecked[0].shape[0])
            out["score_without_photometric"] = evaluation.evaluate_point_cloud(unchecked[0], gt, **kw)
        if low_grid_points is not None:
            out["upsample"]["score_low_grid"] = evaluation.evaluate_point_cloud(low_grid_points, gt, **kw)
            out["upsample"]["score_high_grid"] = out["score_before_cleaning"] if clean else out["score"]
        if mesh_vertices is not None and mesh_vertices.shape[0]:
            out["mesh"]["score"] = evaluation.evaluate_point_cloud(mesh_vertices, gt, **kw)
            import inspect
            from pointmvsnet_amd import mesh_ops
            pitch = args.mesh_sample_pitch
            if pitch is None:                                    # what evaluate_point_cloud thins at: no min_dist is passed above
                pitch = kw.get("min_dist", inspect.signature(evaluation.evaluate_point_cloud).parameters["min_dist"].default)
            samples = mesh_ops.sample_surface(mesh_vertices, faces, pitch)[0]
            out["mesh"]["sample_pitch"], out["mesh"]["samples"] = float(pitch), int(samples.shape[0])
            if samples.shape[0]:
                out["mesh"]["score_sampled"] = evaluation.evaluate_point_cloud(samples, gt, **kw)
            from pointmvsnet_amd import mesh_distance
            out["mesh"]["score_surface"] = mesh_distance.evaluate_mesh(mesh_vertices, faces, gt, pitch=pitch, **kw)
            if unsimplified is not None and unsimplified[1].shape[0]:
                out["mesh"]["score_surface_before_simplification"] = mesh_distance.evaluate_mesh(
                    unsimplified[0], unsimplified[1], gt, pitch=pitch, **kw)
    if args.gt_mesh and points.shape[0]:
        from pointmvsnet_amd import mesh_distance
        kw = {}
        if args.obs_mask:
            mask, bb_min, res = io.load_dtu_obs_mask(args.obs_mask)
            kw.update(obs_mask=torch.from_numpy(mask), bb_min=bb_min, res=res)
        if args.plane:
            kw.update(plane=io.load_dtu_plane(args.plane))
        surface_vertices, surface_faces = mesh_distance.load_ply_surface(args.gt_mesh, dev)
        out["score_gt_mesh"] = mesh_distance.evaluate_point_cloud_on_mesh(points, surface_vertices, surface_faces, **kw)
    print(json.dumps(out))
    if (args.gt or args.gt_mesh) and args.depth_errors:
        interval = float(dataset[0]["cam_params_list"][0, 1, 3, 1]) * INTERVAL_SCALE.get(args.name, 1.0)
        thresholds = [interval, 3.0 * interval]
        line = {"scan": args.scan, "name": args.name, "depth_interval": interval}
        if args.gt_mesh:                                         # the surface wins over the cloud: that is what it is for
            import numpy as np
            gt_vertices, _, _, gt_faces = io.load_ply_mesh(args.gt_mesh)
            if gt_faces is None or not len(gt_faces):
                ap.error("--gt-mesh: %s has no faces" % args.gt_mesh)
            gt = torch.from_numpy(np.ascontiguousarray(gt_vertices, dtype=np.float32)).to(dev)
            kw = {"gt_faces": torch.from_numpy(np.ascontiguousarray(gt_faces).astype(np.int64)).to(dev)}
            line.update(ground_truth="mesh", gt_vertices=int(gt.shape[0]), gt_faces=int(len(gt_faces)))
        else:
            kw = {"splat": args.splat}
            line.update(ground_truth="cloud", splat=args.splat)
        line["depth_errors_raw"] = acc.depth_errors(gt, thresholds, filtered=False, **kw)
        acc.clean_depth = None
        line["depth_errors_filtered"] = acc.depth_errors(gt, thresholds, filtered=True, **kw)
        if clean_depth is not None:
            acc.clean_depth = clean_depth
            line["depth_errors_cleaned"] = acc.depth_errors(gt, thresholds, filtered=True, **kw)
        print(json.dumps(line))


if __name__ == "__main__":
    main()
