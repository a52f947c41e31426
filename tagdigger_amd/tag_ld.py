#!/usr/bin/env python3
"""Pairwise LD of the markers from genotype calls: the step behind tag_calls, beside tag_relate.  For every pair of
markers it takes the correlation r^2 of their calls over the samples called at both and writes the pairs that reach
--min-r2; from those pairs, the groups of markers that hang together (linkage groups, bins of co-segregating markers,
tags that tag_pairs made twice) and a pruned set in which no two markers are in LD.

    python -m tagdigger_amd.tag_ld -i calls.csv -o ld_pairs.csv --groups groups.csv --keep keep.txt
    python -m tagdigger_amd.tag_ld -i calls.csv -o ld_pairs.csv --min-r2 0.5 --min-shared 100 --td-backend host

The input is tag_calls' -o file (writeGenoCalls' layout: samples in rows, markers in columns, 0 / 1 / 2, blank for
missing).  -o has one row per pair in LD; --groups one row per marker; --keep the names of the pruned set, one per line:
what -k/--tokeep of tag_calls and of the counting script reads.
"""
import argparse
import sys

from . import tagdigger_fun as tf
from .tag_relate import read_calls


def build_parser():
    ap = argparse.ArgumentParser(description="Pairwise marker LD (r^2), linkage groups and LD pruning from genotype calls")
    ap.add_argument("-i", "--calls", required=True, metavar="FILE", help="genotype CSV of tag_calls (samples x markers; blank: missing)")
    ap.add_argument("-o", "--output", required=True, metavar="FILE", help="pairs CSV to write (one row per pair of markers in LD)")
    ap.add_argument("--groups", metavar="FILE", help="groups CSV to write (one row per marker: group, size, degree, called, kept)")
    ap.add_argument("--keep", metavar="FILE", help="names of the LD-pruned markers to write, one per line (for -k/--tokeep)")
    ap.add_argument("--min-r2", type=float, default=0.8, help="a pair with at least this r^2 is in LD")
    ap.add_argument("--min-shared", type=int, default=50, help="... when at least this many samples are called at both")
    ap.add_argument("--td-device", type=int, default=0, help="GPU to run on")
    ap.add_argument("--td-backend", choices=["gpu", "host"], default="gpu", help="host: numpy on the CPU")
    return ap


def write_keep(filename, result, keep=None):
    """The kept marker names, one per line (readMarkerNames' format)."""
    keep = tf.ld_prune(result) if keep is None else keep
    with open(filename, "w") as fh:
        for name, k in zip(result.markers, keep):
            if k:
                fh.write(name + "\n")


def summary_line(result, groups, keep):
    return "Markers: {} Participating: {} Edges: {} Groups: {} Kept: {}".format(
        len(result.markers), result.stats["used"], len(result.edges), int(groups.max()) if len(groups) else 0,
        int(keep.sum()))


def main(argv=None):
    args = build_parser().parse_args(argv)
    _, markers, calls = read_calls(args.calls)
    result = tf.marker_ld(calls, markers, min_r2=args.min_r2, min_shared=args.min_shared, device=args.td_device,
                          backend=args.td_backend)
    groups, keep = tf.ld_groups(result), tf.ld_prune(result)
    tf.writeLDPairs(args.output, result)
    if args.groups is not None:
        tf.writeLDGroups(args.groups, result, groups, keep)
    if args.keep is not None:
        write_keep(args.keep, result, keep)
    print(summary_line(result, groups, keep))
    return 0


if __name__ == "__main__":
    sys.exit(main())
