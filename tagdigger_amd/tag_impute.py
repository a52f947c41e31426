#!/usr/bin/env python3
"""LD-kNN imputation of the missing genotype calls: the step behind tag_calls, beside tag_relate and tag_ld.  GBS calls
are full of holes; GWAS, PCA and mapping software wants a full matrix.  For a missing call it takes the markers most in LD
with that marker, finds the samples most alike over those markers, and lets them vote; a cell on which they do not agree
stays missing.  It needs no genome and no map: the calls and their pairwise LD are all it reads.

    python -m tagdigger_amd.tag_impute -i calls.csv -o imputed.csv --stats impute_stats.csv
    python -m tagdigger_amd.tag_impute -i calls.csv -o imputed.csv -l 30 -k 8 --min-conf 0.7 --check 0.05 --seed 1

The input is tag_calls' -o file (writeGenoCalls' layout: samples in rows, markers in columns, 0 / 1 / 2, blank for
missing) and -o has the same layout.  --stats has one row per marker: missing, imputed, no_donor, undecided, neighbours.
--check hides that share of the called cells first, imputes them, and prints the table of true class against outcome:
the way to choose -l, -k, --min-overlap and --min-conf for one's own data.
"""
import argparse
import sys

from . import tagdigger_fun as tf
from .tag_relate import read_calls


def add_tuning(ap, prefix="", min_r2="--min-r2", ld_min_shared=True):
    """The options of the method, shared with tag_calls (which spells -l and -k out: -k is its --tokeep)."""
    ap.add_argument(*(["-l"] if not prefix else []), "--" + prefix + "neighbours", dest="impute_l", type=int, default=20,
                    help="markers most in LD with a marker that stand in for it")
    ap.add_argument(*(["-k"] if not prefix else []), "--" + prefix + "voters", dest="impute_k", type=int, default=10,
                    help="samples most alike over those markers that vote")
    ap.add_argument("--min-overlap", type=int, default=4, help="a sample votes when it shares at least this many called neighbours with the cell's sample")
    ap.add_argument("--min-conf", type=float, default=0.6, help="a cell is filled when the winning class has at least this share of the votes' weight")
    ap.add_argument(min_r2, dest="impute_min_r2", type=float, default=0.5, help="a marker's neighbours have at least this r^2 with it")
    if ld_min_shared:
        ap.add_argument("--ld-min-shared", type=int, default=50, help="... over at least this many samples called at both")


def build_parser():
    ap = argparse.ArgumentParser(description="LD-kNN imputation of missing genotype calls")
    ap.add_argument("-i", "--calls", required=True, metavar="FILE", help="genotype CSV of tag_calls (samples x markers; blank: missing)")
    ap.add_argument("-o", "--output", required=True, metavar="FILE", help="genotype CSV to write, the holes filled where the vote is clear")
    ap.add_argument("--stats", metavar="FILE", help="per-marker CSV to write: missing, imputed, no_donor, undecided, neighbours")
    add_tuning(ap)
    ap.add_argument("--check", type=float, metavar="SHARE", help="hide this share of the called cells, impute them and print true class x outcome")
    ap.add_argument("--seed", type=int, default=0, help="--check: the seed of the draw")
    ap.add_argument("--td-device", type=int, default=0, help="GPU to run on")
    ap.add_argument("--td-backend", choices=["gpu", "host"], default="gpu", help="host: numpy on the CPU")
    return ap


def tuning(args):
    return dict(l=args.impute_l, k=args.impute_k, min_overlap=args.min_overlap, min_conf=args.min_conf, min_r2=args.impute_min_r2,
                ld_min_shared=args.ld_min_shared)


def write_calls(filename, samples, markers, calls):
    """The matrix through tag_calls' genotype writer, every marker."""
    import numpy as np
    tf.writeGenoCalls(filename, tf.GenoResult(list(markers), list(samples), calls, {}, np.ones(len(markers), dtype=bool), None),
                      passing_only=False)


def summary_line(result):
    s = result.stats.sum(axis=0, dtype="uint64")
    return "Markers: {} Missing: {} Imputed: {} No donor: {} Undecided: {}".format(len(result.markers), *(int(x) for x in s))


def check_lines(table):
    lines = ["truth,as_0,as_1,as_2,left_missing"]
    return lines + ["{},{},{},{},{}".format(g, *(int(x) for x in table[g])) for g in range(3)]


def main(argv=None):
    args = build_parser().parse_args(argv)
    samples, markers, calls = read_calls(args.calls)
    kw = dict(tuning(args), device=args.td_device, backend=args.td_backend)
    result = tf.impute_calls(calls, markers, **kw)
    write_calls(args.output, samples, markers, result.calls)
    if args.stats is not None:
        tf.writeImputeStats(args.stats, result)
    print(summary_line(result))
    if args.check is not None:
        table = tf.impute_check(calls, markers, hide_ppm=tf._ppm(args.check, 0, 1000000, "--check"), seed=args.seed, **kw)
        print("\n".join(check_lines(table)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
