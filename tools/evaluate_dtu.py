"""Score a fused point cloud against a scan's ground-truth cloud (pointmvsnet_amd/evaluation.py): DTU accuracy / completeness.

    python tools/evaluate_dtu.py --data OUT/scan9/final3d_model.ply --gt Points/stl/stl009_total.ply \
        [--obs-mask ObsMask/ObsMask9_10.mat --plane ObsMask/Plane9.mat] [--min-dist 0.2] [--max-dist 20] [--no-thin]
    python tools/evaluate_dtu.py --data mesh.ply --data-mesh --gt Points/stl/stl009_total.ply [--pitch 0.2] ...
    python tools/evaluate_dtu.py --data OUT/scan9/final3d_model.ply --gt-mesh surface.ply [--pitch 0.2] ...

Prints the dict of ``evaluate_point_cloud`` as one JSON line.  With ``--data-mesh`` the data file is read as a mesh
(``utils.io.load_ply_mesh``) and scored by its surface (pointmvsnet_amd/mesh_distance.py, ``evaluate_mesh``: samples at
``--pitch`` one way, exact point-to-mesh distances the other).  With ``--gt-mesh FILE`` the cloud is scored against a
ground-truth surface (``evaluate_point_cloud_on_mesh``, the surface sampled at ``--pitch`` for completeness).  The .mat files
need SciPy.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True, help="the reconstructed cloud (binary little-endian PLY)")
    ap.add_argument("--gt", default=None, help="the ground-truth cloud (PLY)")
    ap.add_argument("--data-mesh", action="store_true", help="--data is a mesh (PLY with faces): score its surface")
    ap.add_argument("--gt-mesh", default=None, help="a ground-truth surface (PLY with faces) instead of --gt")
    ap.add_argument("--pitch", type=float, default=0.2, help="--data-mesh / --gt-mesh: the pitch of the surface samples")
    ap.add_argument("--seed", type=int, default=0, help="--data-mesh / --gt-mesh: the seed of the surface samples")
    ap.add_argument("--obs-mask", default=None, help="DTU's ObsMask<scan>_10.mat")
    ap.add_argument("--plane", default=None, help="DTU's Plane<scan>.mat")
    ap.add_argument("--min-dist", type=float, default=0.2)
    ap.add_argument("--max-dist", type=float, default=20.0)
    ap.add_argument("--no-thin", action="store_true")
    ap.add_argument("--device", default=None)
    args = ap.parse_args(argv)
    if (args.gt is None) == (args.gt_mesh is None):
        ap.error("give one of --gt and --gt-mesh")
    if args.data_mesh and args.gt_mesh:
        ap.error("--data-mesh needs --gt: mesh-to-mesh distances are out of scope")
    return args


def score(args, device=None):
    """The dict that ``main`` prints."""
    device = args.device if device is None else device
    if args.data_mesh:
        from pointmvsnet_amd import mesh_distance
        return mesh_distance.evaluate_mesh_ply(args.data, args.gt, obs_mask_mat=args.obs_mask, plane_mat=args.plane,
                                               pitch=args.pitch, max_dist=args.max_dist, seed=args.seed, device=device)
    if args.gt_mesh:
        from pointmvsnet_amd import mesh_distance
        return mesh_distance.evaluate_ply_on_mesh(args.data, args.gt_mesh, obs_mask_mat=args.obs_mask, plane_mat=args.plane,
                                                  gt_pitch=args.pitch, min_dist=args.min_dist, max_dist=args.max_dist,
                                                  thin=not args.no_thin, seed=args.seed, device=device)
    from pointmvsnet_amd import evaluation
    return evaluation.evaluate_ply(args.data, args.gt, obs_mask_mat=args.obs_mask, plane_mat=args.plane,
                                   min_dist=args.min_dist, max_dist=args.max_dist, thin=not args.no_thin, device=device)


def main():
    print(json.dumps(score(parse_args())))


if __name__ == "__main__":
    main()
