"""python -m vision3d_amd.evaluation --labels DIR --results DIR [--ids FILE] [--metrics bbox,bev,3d,aos]
    [--overlaps strict,loose,coco] [--r11]

Evaluates KITTI result files (16 fields, with score) against label_2 files of the same frame ids and prints the summary.  Frame
ids: one per line of --ids, else every result file's name; a listed frame without a result file has no detections."""
import argparse
import os
import sys

from ..dataset import kitti as K
from .kitti import KittiEvaluator


def parse_args(argv=None):
    """The command line -> (parser, args), args.metrics and args.overlaps as tuples of names."""
    ap = argparse.ArgumentParser(prog="python -m vision3d_amd.evaluation", description=__doc__.split("\n\n")[1])
    ap.add_argument("--labels", required=True, help="directory of ground-truth label files (label_2)")
    ap.add_argument("--results", required=True, help="directory of result files")
    ap.add_argument("--ids", help="file with one frame id per line (default: every result file)")
    ap.add_argument("--metrics", default="bev,3d", help="comma list of bbox, bev, 3d, aos, printed in this order (default: bev,3d)")
    ap.add_argument("--overlaps", default="strict,loose",
                    help="comma list of strict, loose, coco (the COCO-style AP over ten minimum overlaps), printed in this order "
                         "(default: strict,loose)")
    ap.add_argument("--r11", action="store_true", help="also print AP on the 11 recall positions")
    args = ap.parse_args(argv)
    args.metrics = tuple(m.strip() for m in args.metrics.split(",") if m.strip())
    args.overlaps = tuple(o.strip() for o in args.overlaps.split(",") if o.strip())
    return ap, args


def main(argv=None):
    ap, args = parse_args(argv)
    if args.ids:
        ids = [ln.strip() for ln in open(args.ids) if ln.strip()]
    else:
        ids = sorted(f[:-4] for f in os.listdir(args.results) if f.endswith(".txt"))
    if not ids:
        ap.error("no frames to evaluate")
    try:
        ev = KittiEvaluator(metrics=args.metrics, overlaps=args.overlaps)
    except ValueError as e:
        ap.error(str(e))
    for i in ids:
        name = f"{int(i):06d}" if i.isdigit() else i
        res = os.path.join(args.results, name + ".txt")
        ev.add_frame(K.read_labels(os.path.join(args.labels, name + ".txt")), K.read_labels(res if os.path.exists(res) else os.devnull))
    ev.compute()
    print(ev.summary(r11=args.r11))
    return 0


if __name__ == "__main__":
    sys.exit(main())
