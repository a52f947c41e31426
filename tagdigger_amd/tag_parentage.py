#!/usr/bin/env python3
"""Parent pairs from genotype calls by Mendelian exclusion: the step behind tag_calls for a breeding population.  For
every offspring it finds the candidate parents by the pair test (hardly any opposing homozygotes), counts for every pair
of candidates the markers at which the three calls break Mendel's rules, and reports the pair that fits, whether a second
pair fits as well, or the one parent that can be named.

    python -m tagdigger_amd.tag_parentage -i calls.csv -o parentage.csv --trios trios.csv
    python -m tagdigger_amd.tag_parentage -i calls.csv -o parentage.csv --offspring seedlings.txt --parents founders.txt --no-selfing
    python -m tagdigger_amd.tag_parentage -i calls.csv -o parentage.csv --max-trio-err 0.05 --min-shared 200 --td-backend host

The input is tag_calls' -o file (writeGenoCalls' layout: samples in rows, markers in columns, 0 / 1 / 2, blank for
missing).  --offspring and --parents name files with one sample name a line (default: every sample).  -o has one row per
offspring; --trios one row per ranked trio.  The thresholds are yours to set for the error rate of your calls: no accuracy
is promised.
"""
import argparse
import sys

from . import tagdigger_fun as tf
from .tag_relate import read_calls


def build_parser():
    ap = argparse.ArgumentParser(description="Parent pairs of the samples by Mendelian trio counts from genotype calls")
    ap.add_argument("-i", "--calls", required=True, metavar="FILE", help="genotype CSV of tag_calls (samples x markers; blank: missing)")
    ap.add_argument("-o", "--output", required=True, metavar="FILE", help="parentage CSV to write (one row per offspring)")
    ap.add_argument("--offspring", metavar="FILE", help="names of the samples to find parents for, one per line (default: all)")
    ap.add_argument("--parents", metavar="FILE", help="names of the samples that may be parents, one per line (default: all)")
    ap.add_argument("--max-pair-err", type=float, default=0.03, help="a candidate parent is an opposing homozygote at no larger a share of the shared markers")
    ap.add_argument("--max-trio-err", type=float, default=0.03, help="a trio passes with no larger a share of Mendelian errors")
    ap.add_argument("--min-shared", type=int, default=50, help="... over at least this many markers called in all of them")
    ap.add_argument("--max-candidates", type=int, default=32, help="candidate parents kept per offspring (at most 128)")
    ap.add_argument("--top", type=int, default=2, help="ranked trios kept per offspring (at most 8)")
    ap.add_argument("--no-selfing", action="store_true", help="a sample is not paired with itself")
    ap.add_argument("--trios", metavar="FILE", help="trios CSV to write (one row per ranked trio)")
    ap.add_argument("--td-device", type=int, default=0, help="GPU to run on")
    ap.add_argument("--td-backend", choices=["gpu", "host"], default="gpu", help="host: numpy on the CPU")
    return ap


def read_names(path):
    """The names of a file with one name a line (blank lines skipped); None for no file."""
    if path is None:
        return None
    with open(path) as fh:
        return [line.strip() for line in fh if line.strip()]


def summary_line(result):
    return "Offspring: {} Trio: {} Ambiguous: {} Single: {} None: {}".format(len(result.offspring), *result.counts())


def main(argv=None):
    args = build_parser().parse_args(argv)
    samples, _, calls = read_calls(args.calls)
    result = tf.parentage(calls, samples, offspring=read_names(args.offspring), parents=read_names(args.parents),
                          max_pair_err=args.max_pair_err, max_trio_err=args.max_trio_err, min_shared=args.min_shared,
                          max_candidates=args.max_candidates, top=args.top, selfing=not args.no_selfing, device=args.td_device,
                          backend=args.td_backend)
    tf.writeParentage(args.output, result)
    if args.trios is not None:
        tf.writeTrios(args.trios, result)
    print(summary_line(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
