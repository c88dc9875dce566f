"""Score a fused point cloud against a scan's ground-truth cloud (pointmvsnet_amd/evaluation.py): DTU accuracy / completeness.

    python tools/evaluate_dtu.py --data OUT/scan9/final3d_model.ply --gt Points/stl/stl009_total.ply \
        [--obs-mask ObsMask/ObsMask9_10.mat --plane ObsMask/Plane9.mat] [--min-dist 0.2] [--max-dist 20] [--no-thin]

Prints the dict of ``evaluate_point_cloud`` as one JSON line.  The .mat files need SciPy.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True, help="the reconstructed cloud (binary little-endian PLY)")
    ap.add_argument("--gt", required=True, help="the ground-truth cloud (PLY)")
    ap.add_argument("--obs-mask", default=None, help="DTU's ObsMask<scan>_10.mat")
    ap.add_argument("--plane", default=None, help="DTU's Plane<scan>.mat")
    ap.add_argument("--min-dist", type=float, default=0.2)
    ap.add_argument("--max-dist", type=float, default=20.0)
    ap.add_argument("--no-thin", action="store_true")
    ap.add_argument("--device", default=None)
    args = ap.parse_args()
    from pointmvsnet_amd import evaluation
    out = evaluation.evaluate_ply(args.data, args.gt, obs_mask_mat=args.obs_mask, plane_mat=args.plane,
                                  min_dist=args.min_dist, max_dist=args.max_dist, thin=not args.no_thin, device=args.device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
