#!/usr/bin/env python3
"""Record what the reference geometry module computes on the synthetic RGB-D scenes, as the fixture of
tests/test_reference_parity_cpu.py (tests/golden/reference_geometry.npz).

The reference module (its ``pkg/geometry_utils.py``; numpy + scipy only) is loaded by file path and only
run: the fixture holds its outputs, none of its code. Per scene seed s: ``pcd_s`` (``_get_pcd_from_mask``),
``edge_s`` (``_find_point_cloud_edge``), ``curv_s`` (mean, max of ``_calculate_spline_curvature`` on scipy's
``splprep`` fit of the x-sorted edge points); ``early`` holds (mean, max, number of spline points) of
``compute_curvature_profile`` on the two early-exit inputs of the test.

usage: python scripts/record_reference_geometry.py --reference PATH/TO/geometry_utils.py [--out FILE]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEEDS = range(6)


def early_exit_masks():
    col = np.zeros((480, 640), np.uint8)
    col[100:250, 320] = 1  # >= 100 points but a zero-width x range -> no edge points
    return np.zeros((480, 640), np.uint8), col


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of the reference's geometry_utils.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "reference_geometry.npz"))
    args = ap.parse_args()
    from scipy.interpolate import splprep

    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K, make_scene
    spec = importlib.util.spec_from_file_location("rdp_reference_geometry_utils", args.reference)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for seed in SEEDS:
        sc = make_scene(seed)
        pcd = ref._get_pcd_from_mask(sc.mask, sc.depth, DEFAULT_K, 0.001)
        edge = ref._find_point_cloud_edge(pcd)
        pts = np.ascontiguousarray(edge[np.argsort(edge[:, 0])])
        tck, _ = splprep([pts[:, 0], pts[:, 1], pts[:, 2]], s=0.1, k=3)
        out[f"pcd_{seed}"], out[f"edge_{seed}"] = pcd, edge
        out[f"curv_{seed}"] = np.array(ref._calculate_spline_curvature(tck), np.float64)
    depth = np.full((480, 640), 500, np.uint16)
    early = []
    for mask in early_exit_masks():
        r = ref.compute_curvature_profile(mask, depth, DEFAULT_K, 0.001)
        early.append([r.mean_curvature, r.max_curvature, len(r.spline_points)])
    out["early"] = np.array(early, np.float64)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
