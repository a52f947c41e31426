#!/usr/bin/env python3
"""Pairwise sample relations from genotype calls: the step behind tag_calls.  For every pair of samples it counts how
often call a in one meets call b in the other, and writes the IBS counts, the IBS distance, the KING-robust kinship and
whether the two look like one plant (a duplicate well).

    python -m tagdigger_amd.tag_relate -i calls.csv -o pairs.csv --matrix dist.csv
    python -m tagdigger_amd.tag_relate -i calls.csv -o pairs.csv --max-dist 0.05 --min-shared 200 --td-backend host

The input is tag_calls' -o file (writeGenoCalls' layout: samples in rows, markers in columns, 0 / 1 / 2, blank for
missing).  -o has one row per pair of samples; --matrix the samples x samples distances.
"""
import argparse
import csv
import sys

from . import tagdigger_fun as tf


def build_parser():
    ap = argparse.ArgumentParser(description="Pairwise sample relations (IBS distance, kinship, duplicates) from genotype calls")
    ap.add_argument("-i", "--calls", required=True, metavar="FILE", help="genotype CSV of tag_calls (samples x markers; blank: missing)")
    ap.add_argument("-o", "--output", required=True, metavar="FILE", help="pairs CSV to write (one row per pair of samples)")
    ap.add_argument("--matrix", metavar="FILE", help="distance matrix CSV to write (samples x samples)")
    ap.add_argument("--max-dist", type=float, default=0.02, help="a pair at most this far apart is a duplicate")
    ap.add_argument("--min-shared", type=int, default=50, help="... when at least this many markers are called in both")
    ap.add_argument("--td-device", type=int, default=0, help="GPU to run on")
    ap.add_argument("--td-backend", choices=["gpu", "host"], default="gpu", help="host: numpy on the CPU")
    return ap


def read_calls(path):
    """(sample names, marker names, uint8 matrix) of a CSV written by writeGenoCalls."""
    import numpy as np
    codes = {"0": 0, "1": 1, "2": 2, "": tf.GENO_MISSING}
    with open(path, newline="") as fh:
        rows = csv.reader(fh)
        header = next(rows, None)
        if header is None or len(header) < 1 or header[0] != "":
            raise Exception("{}: not a genotype file (an empty first header cell, then marker names, expected).".format(path))
        samples, data = [], []
        for row in rows:
            if row:
                if len(row) != len(header):
                    raise Exception("{}: sample {} has {} calls, the header names {} markers.".format(
                        path, row[0], len(row) - 1, len(header) - 1))
                try:
                    data.append([codes[x.strip()] for x in row[1:]])
                except KeyError as err:
                    raise Exception("{}: sample {} has the call {!r}; 0, 1, 2 or blank expected.".format(path, row[0], err.args[0]))
                samples.append(row[0])
    return samples, header[1:], np.array(data, dtype=np.uint8).reshape(len(samples), len(header) - 1)


def summary_line(result):
    S = len(result.samples)
    return "Samples: {} Markers: {} Pairs: {} Duplicates: {}".format(S, result.stats["used"], S * (S - 1) // 2, len(result.duplicates))


def main(argv=None):
    args = build_parser().parse_args(argv)
    samples, _, calls = read_calls(args.calls)
    result = tf.sample_relations(calls, samples, max_dist=args.max_dist, min_shared=args.min_shared, device=args.td_device,
                                 backend=args.td_backend)
    tf.writeRelations(args.output, result)
    if args.matrix is not None:
        tf.writeDistanceMatrix(args.matrix, result)
    print(summary_line(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
