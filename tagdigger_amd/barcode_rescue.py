#!/usr/bin/env python3
"""Tag counts with the reads whose barcode is one or two bases off brought back: every pass over a FASTQ file drops a
read whose first bases are not exactly a barcode + cut site, so one sequencing error or one N in the first 9 to 14
bases loses the whole read.

    python -m tagdigger_amd.barcode_rescue -e PstI --MergedTags markers.csv -b key.csv -o counts.csv --stats bcrescue.csv
    python -m tagdigger_amd.barcode_rescue -e PstI --MergedTags markers.csv -b key.csv -o counts.csv --max-mismatch 2 --rescued-out rescued.csv --rows-out rows.csv

Per library of the key file the exact counts (find_tags_fastq) and the rescued counts (rescue_barcodes_fastq: the
nearest barcode + cut site within --max-mismatch substitutions, when the entries of exactly one barcode are that near,
then the counter's tag step) are taken, folded into sample rows and written as the counter writes them: exact +
rescued to -o, which reads straight into tag_calls -i; the rescued part and the rescued reads per barcode on request.
One line per library names the classes, and one more warns when two barcodes of the set lie no farther apart than
--max-mismatch: exact reads of one sample are then one error from rescue into another.
"""
import argparse
import csv
import sys

from . import tagdigger_fun as tf
from .tagdigger_script import FILE_OPTIONS, TAG_FORMATS, checked, cut_site, tag_format


def build_parser():
    ap = argparse.ArgumentParser(description="Tag counts per sample with the reads one or two substitutions from a barcode + cut site added")
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
    ap.add_argument("--max-mismatch", type=int, choices=[1, 2], default=1, help="substitutions a rescued read may lie from its barcode + cut site")
    ap.add_argument("--maxreads", type=float, default=5e9, help="stop after this many reads of a library")
    ap.add_argument("-o", "--output", required=True, metavar="FILE", help="samples x tags CSV to write: exact + rescued")
    ap.add_argument("--rescued-out", metavar="FILE", help="samples x tags CSV of the rescued counts alone")
    ap.add_argument("--rows-out", metavar="FILE", help="CSV to write: one row per library and barcode with the reads rescued at 1 and at 2")
    ap.add_argument("--stats", metavar="FILE", help="CSV to write: one row per library with the classes")
    ap.add_argument("--td-device", type=int, default=0, help="GPU to run on")
    ap.add_argument("--td-backend", choices=["gpu", "host"], default="gpu", help="host: both matrices by the rule in Python on the CPU")
    return ap


def library_counts(fqfile, barcodes, sequences, site, maxreads, max_mismatch, device, backend):
    """(exact matrix, rescued matrix, statistics) of one library, the matrices as lists."""
    if backend == "host":
        exact = tf._rescue_host(fqfile, barcodes, sequences, site, maxreads, 1)[3]
    else:
        exact = tf.find_tags_fastq(fqfile, barcodes, sequences, cutsite=site, maxreads=maxreads, device=device, progress=False)
    rescued, stats = tf.rescue_barcodes_fastq(fqfile, barcodes, sequences, cutsite=site, maxreads=maxreads, max_mismatch=max_mismatch,
                                              device=device, backend=backend)
    return exact, rescued, stats


def stats_line(library, st, backend):
    return "{}: {} reads: {} exact, {} rescued at 1, {} rescued at 2, {} ambiguous, {} none; {} rescued reads with a tag ({})".format(
        library, st["reads"], st["exact"], st["rescued1"], st["rescued2"], st["ambiguous"], st["none"], st["tagged"], backend)


def warning_line(library, st, max_mismatch):
    return ("{}: WARNING: two barcodes lie {} substitution(s) apart, --max-mismatch is {}: exact reads of one sample are one error "
            "from rescue into another").format(library, st["min_entry_distance"], max_mismatch)


def write_rows(filename, libraries, keys, results):
    """One row per library and barcode: Library, Barcode, Sample, rescued1, rescued2 (csv.writer rows)."""
    with open(filename, mode='w', newline='') as fh:
        out = csv.writer(fh)
        out.writerow(["Library", "Barcode", "Sample", "rescued1", "rescued2"])
        for lib, st in zip(libraries, results):
            for barcode, sample, (r1, r2) in zip(keys[lib][0], keys[lib][1], st["row_rescued"]):
                out.writerow([lib, barcode, sample, r1, r2])


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
    rescued, both, results = {}, {}, []
    for f in libraries:
        exact, rescued[f], st = library_counts(f, keys[f][0], sequences, site, args.maxreads, args.max_mismatch, args.td_device, args.td_backend)
        both[f] = [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(exact, rescued[f])]
        results.append(st)
        print(stats_line(f, st, args.td_backend))
        if st["min_entry_distance"] <= args.max_mismatch:
            print(warning_line(f, st, args.max_mismatch))
    for path, per_file in ((args.output, both), (args.rescued_out, rescued)):
        if path is not None:
            samples, counts = tf.combineReadCounts({f: [list(row) for row in m] for f, m in per_file.items()}, keys)
            tf.writeCounts(path, counts, samples, names)
    if args.rows_out is not None:
        write_rows(args.rows_out, libraries, keys, results)
    if args.stats is not None:
        tf.writeBarcodeRescueStats(args.stats, libraries, results)
    return 0


if __name__ == "__main__":
    sys.exit(main())
