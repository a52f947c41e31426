#!/usr/bin/env python3
"""Tag census from the command line: which sequences follow the barcodes of one library, how often, and which of
them the tag list already holds.

    python -m tagdigger_amd.tag_census -f lib.fq.gz -b key.csv -e PstI -o census.csv --top 1000 --known-merged tags.csv

The CSV has the header `Tag sequence,Count,Known tags`; its rows are ordered by count descending, then sequence.
The barcodes are the key file's for this library (tagdigger_script's -b file: FASTQ file, barcode, sample).
"""
import argparse
import csv
import os
import sys

from . import tagdigger_fun as tf
from .tagdigger_script import cut_site


def build_parser():
    ap = argparse.ArgumentParser(description="List the distinct sequences behind the barcodes of one FASTQ library")
    ap.add_argument("-f", "--fastq", required=True, metavar="FILE", help="the library, plain or .gz")
    ap.add_argument("-b", "--barcodefile", required=True, metavar="FILE", help="key file: FASTQ file, barcode, sample")
    site = ap.add_argument_group("restriction site (one of the two)")
    site.add_argument("-e", "--enzyme", choices=sorted(tf.enzymes), help="enzyme whose remnant follows the barcode")
    site.add_argument("-c", "--cutsite", help="that remnant spelled out (IUPAC codes allowed)")
    ap.add_argument("-o", "--output", required=True, metavar="FILE", help="CSV to write")
    ap.add_argument("--taglen", type=int, default=64, help="bases per window, from the cut site's first base (1..64)")
    ap.add_argument("--min-count", type=int, default=1, help="leave out windows seen fewer times")
    ap.add_argument("--top", type=int, default=None, help="keep the N most frequent windows")
    ap.add_argument("--maxreads", type=float, default=5e9, help="stop after this many reads")
    ap.add_argument("--known-merged", metavar="FILE", help="merged tag table whose tags are named in the third column")
    ap.add_argument("--td-device", type=int, default=0, help="GPU to run on")
    ap.add_argument("--td-backend", choices=["gpu", "host"], default="gpu", help="host: a plain dict on the CPU")
    return ap


def library_barcodes(keys, fastq):
    """The barcodes the key file lists for this library: by the name as given, by its base name, or -- the key file
    naming one library only -- that one's."""
    if fastq in keys:
        return keys[fastq][0]
    base = os.path.basename(fastq)
    named = [f for f in keys if os.path.basename(f) == base]
    if len(named) == 1:
        return keys[named[0]][0]
    if len(keys) == 1:
        return next(iter(keys.values()))[0]
    raise Exception("Library {} is not in the barcode file.".format(fastq))


def stats_line(stats):
    return ("Reads: {reads} With barcode and cut site: {barcut} Short: {short} Ambiguous: {ambiguous} "
            "Counted: {counted} Distinct: {distinct}").format(**stats)


def main(argv=None):
    args = build_parser().parse_args(argv)
    site = cut_site(args)
    keys = tf.readBarcodeKeyfile(args.barcodefile)
    if keys is None:
        raise Exception("Problem reading barcode file.")
    known = None
    if args.known_merged is not None:
        known = tf.readTags_Merged(args.known_merged)
        if known is None:
            raise Exception("Problem reading tags.")
    res = tf.tag_census(args.fastq, library_barcodes(keys, args.fastq), cutsite=site, taglen=args.taglen,
                        maxreads=args.maxreads, min_count=args.min_count, top=args.top, known=known,
                        device=args.td_device, backend=args.td_backend)
    names = res[2] if known is not None else [""] * len(res[0])
    with open(args.output, "w", newline="") as fh:
        out = csv.writer(fh)
        out.writerow(["Tag sequence", "Count", "Known tags"])
        out.writerows(zip(res[0], res[1], names))
    print(stats_line(res.stats))
    return 0


if __name__ == "__main__":
    sys.exit(main())
