#!/usr/bin/env python3
"""Tag counts with the reads one or two substitutions from a known tag brought back: the counter drops a read with
one sequencing error or one N inside its tag, and depth per cell is what the genotype calls are made from.

    python -m tagdigger_amd.tag_rescue -e PstI --MergedTags markers.csv -b key.csv -o counts.csv --stats rescue.csv
    python -m tagdigger_amd.tag_rescue -e PstI --MergedTags markers.csv -b key.csv -o counts.csv --max-mismatch 2 --exact-out exact.csv --rescued-out rescued.csv

Per library of the key file the exact counts (find_tags_fastq) and the rescued counts (rescue_tags_fastq: the nearest tag
within --max-mismatch substitutions, when exactly one tag is that near) are taken, folded into sample rows and written
as the counter writes them: exact + rescued to -o, which reads straight into tag_calls -i; each part on request.  One
line per library names the classes, so that the share the rescue brings back is seen for the data at hand.
"""
import argparse
import sys

from . import tagdigger_fun as tf
from .tagdigger_script import FILE_OPTIONS, TAG_FORMATS, checked, cut_site, tag_format


def build_parser():
    ap = argparse.ArgumentParser(description="Tag counts per sample with the reads one or two substitutions from a known tag added")
    site = ap.add_argument_group("restriction site (one of the two)")
    site.add_argument("-e", "--enzyme", choices=sorted(tf.enzymes), help="enzyme whose remnant follows the barcode")
    site.add_argument("-c", "--cutsite", help="that remnant spelled out (IUPAC codes allowed)")
    fmt = ap.add_argument_group("tags (exactly one format)")
    for opt, what in FILE_OPTIONS.items():
        fmt.add_argument("--" + opt, metavar="FILE", help=what)
    ap.add_argument("-k", "--tokeep", metavar="FILE", help="marker names to keep, one per line")
    ap.add_argument("--binaryOnly", choices=["T", "F"], default="F", help="T: drop markers with more than two alleles")
    ap.add_argument("--TASSELkeyFile", metavar="FILE", help="write the key to the TASSEL marker names here")
    ap.add_argument("-b", "--barcodefile", required=True, metavar="FILE", help="key file: FASTQ file, barcode, sample")
    ap.add_argument("--max-mismatch", type=int, choices=[1, 2], default=1, help="substitutions a rescued read may lie from its tag")
    ap.add_argument("--maxreads", type=float, default=5e9, help="stop after this many reads of a library")
    ap.add_argument("-o", "--output", required=True, metavar="FILE", help="samples x tags CSV to write: exact + rescued")
    ap.add_argument("--exact-out", metavar="FILE", help="samples x tags CSV of the exact counts alone")
    ap.add_argument("--rescued-out", metavar="FILE", help="samples x tags CSV of the rescued counts alone")
    ap.add_argument("--stats", metavar="FILE", help="CSV to write: one row per library with the classes")
    ap.add_argument("--td-device", type=int, default=0, help="GPU to run on")
    ap.add_argument("--td-backend", choices=["gpu", "host"], default="gpu", help="host: both matrices by the rule in Python on the CPU")
    return ap


def library_counts(fqfile, barcodes, sequences, site, maxreads, max_mismatch, device, backend):
    """(exact matrix, RescueResult) of one library, the matrices as lists."""
    if backend == "host":
        rescued, stats, positions, exact = tf._rescue_host(fqfile, barcodes, sequences, site, maxreads, max_mismatch)
        return exact, tf.RescueResult(rescued, {k: stats[k] for k in tf.RESCUE_STAT_NAMES}, positions, "host")
    exact = tf.find_tags_fastq(fqfile, barcodes, sequences, cutsite=site, maxreads=maxreads, device=device, progress=False)
    return exact, tf.rescue_tags_fastq(fqfile, barcodes, sequences, cutsite=site, maxreads=maxreads, max_mismatch=max_mismatch, device=device)


def stats_line(library, result):
    st = result.stats
    return "{}: {} reads, {} with barcode + cut site: {} exact, {} rescued at 1, {} rescued at 2, {} ambiguous, {} none ({})".format(
        library, st["reads"], st["barcut"], st["exact"], st["rescued1"], st["rescued2"], st["ambiguous"], st["none"], result.backend)


def main(argv=None):
    args = build_parser().parse_args(argv)
    site = cut_site(args)
    keep = checked(tf.readMarkerNames(args.tokeep), "marker names to keep") if args.tokeep is not None else None
    tags = checked(TAG_FORMATS[tag_format(args)][1](args, keep, args.binaryOnly == "T"), "tags")
    names, sequences = tf.sanitizeTags(tags)
    keys = checked(tf.readBarcodeKeyfile(args.barcodefile), "barcode file")
    libraries = sorted(keys)
    unreadable = [f for f in libraries if not tf.isFastq(f)]
    if unreadable:
        print("Cannot read the following as FASTQ files:")
        print(unreadable)
        raise Exception("Cannot read all FASTQ files.")
    exact, rescued, both, results = {}, {}, {}, []
    for f in libraries:
        exact[f], res = library_counts(f, keys[f][0], sequences, site, args.maxreads, args.max_mismatch, args.td_device, args.td_backend)
        rescued[f] = res.rescued
        both[f] = [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(exact[f], rescued[f])]
        results.append(res)
        print(stats_line(f, res))
    for path, per_file in ((args.output, both), (args.exact_out, exact), (args.rescued_out, rescued)):
        if path is not None:
            samples, counts = tf.combineReadCounts({f: [list(row) for row in m] for f, m in per_file.items()}, keys)
            tf.writeCounts(path, counts, samples, names)
    if args.stats is not None:
        tf.writeRescueStats(args.stats, libraries, results)
    return 0


if __name__ == "__main__":
    sys.exit(main())
