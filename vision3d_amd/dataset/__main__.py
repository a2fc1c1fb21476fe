"""python -m vision3d_amd.dataset --root KITTI/training --ids train.txt --cachedir CACHE [--min-pts 8] [--reduced | --raw]
    [--batch-frames 64]

Builds the GT-sampling database of the frames listed in --ids (one frame id per line) and writes CACHE/database.pkl, the file
`ChainedAugmentation(cfg)` and the reference's `SampleAugmentation` load.  Points come from velodyne_reduced (--reduced, the
default: the clouds cropped to the camera's view) or velodyne (--raw).  An existing database.pkl is kept as it is."""
import argparse
import os
import pickle
import sys
import time

CLASS_NAMES = {0: "Car", 1: "Pedestrian", 2: "Cyclist", -1: "ignored"}


def parse_args(argv=None):
    """The command line -> (parser, args)."""
    ap = argparse.ArgumentParser(prog="python -m vision3d_amd.dataset", description=__doc__.split("\n\n")[1])
    ap.add_argument("--root", required=True, help="KITTI training directory (calib, label_2, velodyne_reduced or velodyne)")
    ap.add_argument("--ids", required=True, help="file with one frame id per line")
    ap.add_argument("--cachedir", required=True, help="directory database.pkl is written to (created if missing)")
    ap.add_argument("--min-pts", type=int, default=8, help="keep an object iff it holds MORE points than this (default: 8)")
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--reduced", dest="reduced", action="store_true", default=True, help="read velodyne_reduced (default)")
    which.add_argument("--raw", dest="reduced", action="store_false", help="read velodyne")
    ap.add_argument("--batch-frames", type=int, default=64, help="frames per device call (default: 64)")
    args = ap.parse_args(argv)
    if args.min_pts < 0 or args.batch_frames < 1:
        ap.error("--min-pts must not be negative and --batch-frames must be positive")
    return ap, args


def main(argv=None):
    ap, args = parse_args(argv)
    from ..core.config import _defaults
    from .database import DatabaseBuilder, build_annotations
    if not os.path.isfile(args.ids):
        ap.error(f"no such id file: {args.ids}")
    ids = [int(ln) for ln in open(args.ids) if ln.strip()]
    if not ids:
        ap.error("no frames listed")
    cfg = _defaults().clone()
    cfg.merge_from_dict(dict(DATA=dict(CACHEDIR=args.cachedir), AUG=dict(MIN_NUM_SAMPLE_PTS=args.min_pts)))
    os.makedirs(args.cachedir, exist_ok=True)
    t0 = time.perf_counter()
    try:
        annotations = build_annotations(args.root, ids, reduced=args.reduced)
    except FileNotFoundError as e:
        ap.error(str(e))
    builder = DatabaseBuilder(cfg, annotations, batch_frames=args.batch_frames)
    with open(builder.fpath, "rb") as f:
        database = pickle.load(f)
    for c in sorted(database, key=lambda c: (c < 0, c)):
        items = database[c]
        objects, points = (f"{n:,}".replace(",", " ") for n in (len(items), sum(len(it["points"]) for it in items)))
        print(f"{CLASS_NAMES.get(int(c), int(c))}: {objects} objects, {points} points")
    print(f"{len(ids)} frames, {time.perf_counter() - t0:.1f} s -> {builder.fpath}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
