#!/usr/bin/env python3
"""Markers from a census, without a reference genome: the tags of a library that differ from exactly one other tag at
exactly one base (the UNEAK network filter), written as a merged tag table.

    python -m tagdigger_amd.tag_pairs -i census.csv -o markers.csv
    python -m tagdigger_amd.tag_pairs -f lib.fq.gz -b key.csv -e PstI -o markers.csv --min-count 5

The input is one or more CSVs written by tag_census (their counts are summed by sequence), or a library to take the
census of first.  The output has the header `Marker name,Tag sequence,Count 0,Count 1`: readTags_Merged, the counter's
--MergedTags and writeMarkerDatabase's readers take it as it is.
"""
import argparse
import csv
import sys

from . import tagdigger_fun as tf
from .tag_census import library_barcodes
from .tagdigger_script import cut_site


def build_parser():
    ap = argparse.ArgumentParser(description="Pair the tags of a census that differ at one base into biallelic markers")
    ap.add_argument("-i", "--census", action="append", metavar="FILE", help="census CSV of tag_census (may be repeated)")
    ap.add_argument("-f", "--fastq", metavar="FILE", help="a library to take the census of, plain or .gz")
    ap.add_argument("-b", "--barcodefile", metavar="FILE", help="key file: FASTQ file, barcode, sample (with -f)")
    site = ap.add_argument_group("restriction site (with -f, one of the two)")
    site.add_argument("-e", "--enzyme", choices=sorted(tf.enzymes), help="enzyme whose remnant follows the barcode")
    site.add_argument("-c", "--cutsite", help="that remnant spelled out (IUPAC codes allowed)")
    ap.add_argument("--taglen", type=int, default=64, help="with -f: bases per window (1..64)")
    ap.add_argument("--maxreads", type=float, default=5e9, help="with -f: stop after this many reads")
    ap.add_argument("-o", "--output", required=True, metavar="FILE", help="merged tag table to write")
    ap.add_argument("--min-count", type=int, default=2, help="tags seen fewer times do not take part")
    ap.add_argument("--min-ratio", type=float, default=0.03,
                    help="an edge is cut when its rarer tag has less than this share of the commoner one's count")
    ap.add_argument("--prefix", default="Mrkr", help="marker names are this and a number")
    ap.add_argument("--numdig", type=int, default=7, help="digits of that number")
    ap.add_argument("--td-device", type=int, default=0, help="GPU to run on")
    ap.add_argument("--td-backend", choices=["gpu", "host"], default="gpu", help="host: plain dicts on the CPU")
    return ap


def read_census(paths):
    """{sequence: count} summed over census CSVs (header `Tag sequence,Count,...`), all of one tag length."""
    census = {}
    for path in paths:
        with open(path, newline="") as fh:
            rows = csv.reader(fh)
            header = next(rows, None)
            if header is None or header[:2] != ["Tag sequence", "Count"]:
                raise Exception("{}: not a tag_census file (header 'Tag sequence,Count,...' expected).".format(path))
            for row in rows:
                if row:
                    seq = row[0].strip().upper()
                    census[seq] = census.get(seq, 0) + int(row[1])
    lengths = sorted({len(s) for s in census})
    if len(lengths) > 1:
        raise Exception("The census files hold tags of different lengths ({}); run tag_census with one --taglen.".format(
            ", ".join(str(n) for n in lengths)))
    return census


def stats_line(stats):
    return "Tags: {tags} Edges: {edges} Kept: {kept} Hubs: {hubs} Pairs: {pairs}".format(**stats)


def main(argv=None):
    args = build_parser().parse_args(argv)
    min_count = max(1, args.min_count)
    if (args.census is None) == (args.fastq is None):
        raise Exception("Need either census files (-i) or a library (-f, -b and -e or -c).")
    if args.census is not None:
        census = read_census(args.census)
        entries = sorted(((s, c) for s, c in census.items() if c >= min_count), key=lambda e: (-e[1], e[0]))
        seqs, counts = [e[0] for e in entries], [e[1] for e in entries]
    else:
        if args.barcodefile is None:
            raise Exception("A library (-f) needs its barcode file (-b).")
        site = cut_site(args)
        keys = tf.readBarcodeKeyfile(args.barcodefile)
        if keys is None:
            raise Exception("Problem reading barcode file.")
        res = tf.tag_census(args.fastq, library_barcodes(keys, args.fastq), cutsite=site, taglen=args.taglen,
                            maxreads=args.maxreads, min_count=min_count, device=args.td_device, backend=args.td_backend)
        seqs, counts = res[0], res[1]
    markers = tf.census_markers(seqs, counts, min_ratio=args.min_ratio, prefix=args.prefix, numdig=args.numdig,
                                device=args.td_device, backend=args.td_backend)
    with open(args.output, "w", newline="") as fh:
        out = csv.writer(fh)
        out.writerow(["Marker name", "Tag sequence", "Count 0", "Count 1"])
        for name, merged, (c0, c1) in zip(*markers):
            out.writerow([name, merged, c0, c1])
    print(stats_line(markers.stats))
    return 0


if __name__ == "__main__":
    sys.exit(main())
