#!/usr/bin/env python3
"""Allele dosage calls of polyploid samples from tag counts: tag_calls' sibling for tetraploids, hexaploids and the
like.  Calls every sample at every biallelic marker as 0 .. ploidy copies of allele 1 from the read depths of its two
tags, and drops markers by call rate and minor allele frequency.

    python -m tagdigger_amd.tag_dosage -i counts.csv -o dosage.csv --ploidy 4 --stats stats.csv --min-call-rate 0.8 --min-maf 0.05
    python -m tagdigger_amd.tag_dosage -i counts.csv -o dosage.csv --ploidy 6 --prior flat --min-odds 20 --diploid calls.csv
    python -m tagdigger_amd.tag_dosage -b key.csv --MergedTags markers.csv -e PstI -o dosage.csv --ploidy 4
    python -m tagdigger_amd.tag_dosage -i counts.csv -o dosage.csv --ploidy 4 --vcf dosage.vcf

The input is the counter's CSV (samples in rows, tag names Marker_..._0 / Marker_..._1 in the header), or the
libraries of a key file, which are counted first as tag_calls counts them: every library's barcode rows are folded into
one samples x tags matrix on the device, and the calls are made from that matrix where it lies.  -o has
writeGenoCalls' layout with the values 0 .. ploidy and the markers that pass.  --diploid writes the same markers
diploidised (0 for no copy, 2 for all copies, 1 between): the file tag_relate -i, tag_ld -i, tag_impute -i and
tag_parentage -i read.  --vcf writes the markers that pass as a VCF file (GT with `ploidy` alleles, AD, DP), formatted
on the device from the matrix where it lies; --vcf-positions as for tag_calls.
"""
import argparse
import sys

from . import tagdigger_fun as tf
from .tag_calls import add_vcf_options, count_on_device, read_counts, read_positions, read_tags
from .tagdigger_script import FILE_OPTIONS, checked, cut_site


def build_parser():
    ap = argparse.ArgumentParser(description="Polyploid allele dosage calls and marker filters from the tag counts of biallelic markers")
    ap.add_argument("-i", "--counts", metavar="FILE", help="samples x tags CSV of the counter (instead of -b)")
    ap.add_argument("-b", "--barcodefile", metavar="FILE", help="key file: FASTQ file, barcode, sample; its libraries are counted")
    site = ap.add_argument_group("restriction site (with -b, one of the two)")
    site.add_argument("-e", "--enzyme", choices=sorted(tf.enzymes), help="enzyme whose remnant follows the barcode")
    site.add_argument("-c", "--cutsite", help="that remnant spelled out (IUPAC codes allowed)")
    fmt = ap.add_argument_group("tags (with -b: exactly one format)")
    for opt, what in FILE_OPTIONS.items():
        fmt.add_argument("--" + opt, metavar="FILE", help=what)
    ap.add_argument("-k", "--tokeep", metavar="FILE", help="marker names to keep, one per line")
    ap.add_argument("--binaryOnly", choices=["T", "F"], default="T", help="T (default here): drop markers with more than two alleles")
    ap.add_argument("--TASSELkeyFile", metavar="FILE", help="write the key to the TASSEL marker names here")
    ap.add_argument("--maxreads", type=float, default=5e9, help="with -b: stop after this many reads of a library")
    ap.add_argument("-o", "--output", required=True, metavar="FILE", help="dosage CSV to write (markers that pass)")
    ap.add_argument("--stats", metavar="FILE", help="per-marker statistics CSV to write (every marker)")
    ap.add_argument("--diploid", metavar="FILE", help="diploidised genotype CSV to write (markers that pass; what tag_relate -i and tag_ld -i read)")
    ap.add_argument("--counts-out", metavar="FILE", help="with -b: write the samples x tags counts as well")
    add_vcf_options(ap, likelihoods=False)
    ap.add_argument("--ploidy", type=int, default=4, help="allele copies of every sample, 2 .. 8")
    ap.add_argument("--prior", choices=list(tf.DOSE_PRIORS), default="hwe",
                    help="hwe: Hardy-Weinberg proportions at the marker's allele-1 read share; flat: none")
    ap.add_argument("--err", type=float, default=0.01, help="sequencing error rate")
    ap.add_argument("--min-depth", type=int, default=1, help="fewer reads of both tags together: missing")
    ap.add_argument("--min-odds", type=float, default=10, help="the best dosage less than this many times as probable as the next: missing")
    ap.add_argument("--min-call-rate", type=float, default=0.0, help="drop markers called in a smaller share of the samples")
    ap.add_argument("--min-maf", type=float, default=0.0, help="drop markers with a smaller minor allele frequency")
    ap.add_argument("--td-device", type=int, default=0, help="GPU to run on")
    ap.add_argument("--td-backend", choices=["gpu", "host"], default="gpu", help="host: numpy on the CPU (with -i)")
    return ap


def stats_line(result):
    missing = int((result.calls == tf.DOSE_MISSING).sum())
    return "Samples: {} Markers: {} Ploidy: {} Passed: {} Calls: {} Missing: {}".format(
        len(result.samples), len(result.markers), result.ploidy, result.stats["passed"], result.calls.size - missing, missing)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if (args.counts is None) == (args.barcodefile is None):
        raise Exception("Need either a counts file (-i) or a key file whose libraries are counted (-b, tags and -e or -c).")
    params = dict(ploidy=args.ploidy, prior=args.prior, err=args.err, min_depth=args.min_depth, min_odds=args.min_odds,
                  min_call_rate=args.min_call_rate, min_maf=args.min_maf, device=args.td_device)
    if args.vcf is None and args.vcf_positions is not None:
        raise Exception("--vcf-positions goes with --vcf.")
    positions = read_positions(args.vcf_positions)
    eng = d_counts = sequences = None
    if args.counts is not None:
        if args.counts_out is not None:
            raise Exception("--counts-out goes with counting (-b); -i is that file already.")
        samples, names, counts = read_counts(args.counts)
        backend = args.td_backend
    else:
        if args.td_backend != "gpu":
            raise Exception("Counting runs on the GPU; --td-backend host goes with a counts file (-i).")
        site = cut_site(args)
        names, sequences = read_tags(args)
        keys = checked(tf.readBarcodeKeyfile(args.barcodefile), "barcode file")
        unreadable = [f for f in sorted(keys) if not tf.isFastq(f)]
        if unreadable:
            print("Cannot read the following as FASTQ files:")
            print(unreadable)
            raise Exception("Cannot read all FASTQ files.")
        tf._geno_markers(names)                          # (the alleles are checked before any file is counted)
        eng = tf.default_engine(args.td_device)
        samples, d_counts = count_on_device(eng, keys, sequences, site, args.maxreads)
        counts, backend = d_counts, "gpu"
    try:
        result = tf.call_dosage(counts, samples, names, backend=backend, **params)
        if d_counts is not None and args.counts_out is not None:
            import numpy as np
            host = np.frombuffer(eng.d2h(d_counts.ptr, d_counts.shape[0] * d_counts.shape[1] * 4), dtype=np.uint32)
            tf.writeCounts(args.counts_out, host.reshape(d_counts.shape), samples, names)
        if args.vcf is not None:                         # (while the matrix is on the device)
            tf.writeVCF(args.vcf, result, counts, tagseqs=sequences, positions=positions, passing_only=True, device=args.td_device,
                        backend=backend)
    finally:
        if d_counts is not None:
            eng.dev_free(d_counts.ptr)
    tf.writeDosage(args.output, result, passing_only=True)
    if args.stats is not None:
        tf.writeDosageStats(args.stats, result)
    if args.diploid is not None:
        tf.writeGenoCalls(args.diploid, tf.GenoResult(result.markers, result.samples, result.diploid, result.stats, result.mask,
                                                      result.columns), passing_only=True)
    print(stats_line(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
