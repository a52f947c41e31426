#!/usr/bin/env python3
"""Genotype calls from tag counts: the step behind tag_census -> tag_pairs -> counting.  Calls every sample at every
biallelic marker from the read depths of its two tags, and drops markers by call rate, minor allele frequency and
heterozygosity.

    python -m tagdigger_amd.tag_calls -i counts.csv -o calls.csv --stats stats.csv --min-call-rate 0.8 --min-maf 0.05
    python -m tagdigger_amd.tag_calls -b key.csv --MergedTags markers.csv -e PstI -o calls.csv --hapmap calls.hmp.txt
    python -m tagdigger_amd.tag_calls -i counts.csv -o calls.csv --min-call-rate 0.8 --relations pairs.csv --relations-matrix dist.csv
    python -m tagdigger_amd.tag_calls -i counts.csv -o calls.csv --min-call-rate 0.8 --ld ld_pairs.csv --ld-keep keep.txt --relations pairs.csv --relations-ld-pruned
    python -m tagdigger_amd.tag_calls -i counts.csv -o calls.csv --min-call-rate 0.8 --impute imputed.csv --impute-stats impute_stats.csv
    python -m tagdigger_amd.tag_calls -i counts.csv -o calls.csv --min-call-rate 0.8 --parentage parentage.csv --parentage-parents founders.txt
    python -m tagdigger_amd.tag_calls -b key.csv --SAM tags.sam -e PstI -o calls.csv --vcf calls.vcf --vcf-likelihoods --vcf-positions names

The input is the counter's CSV (samples in rows, tag names Marker_..._0 / Marker_..._1 in the header), or the
libraries of a key file, which are counted first: every library's barcode rows are folded into one samples x tags
matrix on the device, and the calls are made from that matrix where it lies -- it comes to the host only when
--counts-out asks for the CSV as well.  -o has writeDiploidGeno's layout with the markers that pass.  --relations
checks the samples themselves over the markers that pass (tag_relate's table; the calls stay on the device for it).
--ld, --ld-groups and --ld-keep check those markers against each other (tag_ld's files, from the same calls on the
device); --relations-ld-pruned then restricts the relations to the LD-pruned markers.  --impute fills the holes of the
passing markers by LD-kNN imputation (tag_impute's file, from the same calls on the device) and writes them beside -o.
--parentage finds the parent pairs of the samples over the markers that pass (tag_parentage's files and defaults, from the
same calls on the device).  --vcf writes the markers that pass as a VCF file with both read depths of every cell
(GT:AD:DP, with --vcf-likelihoods also GQ:PL), formatted on the device from the matrix and the calls where they lie;
--vcf-positions names reads chromosome and position from marker names chrom-pos-strand, --vcf-positions FILE from a CSV
(Marker name, Chromosome, Position); with the tag file, REF and ALT are the bases of single-base markers.
"""
import argparse
import csv
import sys

from . import tagdigger_fun as tf
from .tagdigger_script import FILE_OPTIONS, TAG_FORMATS, checked, cut_site, tag_format


def build_parser():
    ap = argparse.ArgumentParser(description="Genotype calls and marker filters from the tag counts of biallelic markers")
    ap.add_argument("-i", "--counts", metavar="FILE", help="samples x tags CSV of the counter (instead of -b)")
    ap.add_argument("-b", "--barcodefile", metavar="FILE", help="key file: FASTQ file, barcode, sample; its libraries are counted")
    site = ap.add_argument_group("restriction site (with -b, one of the two)")
    site.add_argument("-e", "--enzyme", choices=sorted(tf.enzymes), help="enzyme whose remnant follows the barcode")
    site.add_argument("-c", "--cutsite", help="that remnant spelled out (IUPAC codes allowed)")
    fmt = ap.add_argument_group("tags (with -b, and for --hapmap: exactly one format)")
    for opt, what in FILE_OPTIONS.items():
        fmt.add_argument("--" + opt, metavar="FILE", help=what)
    ap.add_argument("-k", "--tokeep", metavar="FILE", help="marker names to keep, one per line")
    ap.add_argument("--binaryOnly", choices=["T", "F"], default="T", help="T (default here): drop markers with more than two alleles")
    ap.add_argument("--TASSELkeyFile", metavar="FILE", help="write the key to the TASSEL marker names here")
    ap.add_argument("--maxreads", type=float, default=5e9, help="with -b: stop after this many reads of a library")
    ap.add_argument("-o", "--output", required=True, metavar="FILE", help="genotype CSV to write (markers that pass)")
    ap.add_argument("--stats", metavar="FILE", help="per-marker statistics CSV to write (every marker)")
    ap.add_argument("--hapmap", metavar="FILE", help="HapMap table to write (markers that pass; needs the tag file)")
    ap.add_argument("--counts-out", metavar="FILE", help="with -b: write the samples x tags counts as well")
    add_vcf_options(ap, likelihoods=True)
    ap.add_argument("--relations", metavar="FILE", help="pairs CSV to write: the samples' relations over the markers that pass (see tag_relate)")
    ap.add_argument("--relations-matrix", metavar="FILE", help="distance matrix CSV to write (samples x samples)")
    ap.add_argument("--max-dist", type=float, default=0.02, help="--relations: a pair at most this far apart is a duplicate")
    ap.add_argument("--min-shared", type=int, default=50, help="--relations: ... when at least this many markers are called in both")
    ap.add_argument("--ld", metavar="FILE", help="LD pairs CSV to write: the pairs of passing markers in LD (see tag_ld)")
    ap.add_argument("--ld-groups", metavar="FILE", help="LD groups CSV to write (one row per passing marker)")
    ap.add_argument("--ld-keep", metavar="FILE", help="names of the LD-pruned passing markers to write, one per line")
    ap.add_argument("--min-r2", type=float, default=0.8, help="--ld: a pair with at least this r^2 is in LD")
    ap.add_argument("--ld-min-shared", type=int, default=50, help="--ld: ... when at least this many samples are called at both")
    ap.add_argument("--relations-ld-pruned", action="store_true", help="--relations over the markers that pass AND survive LD pruning")
    ap.add_argument("--impute", metavar="FILE", help="genotype CSV to write as well: the passing markers with their holes filled (see tag_impute)")
    ap.add_argument("--impute-stats", metavar="FILE", help="--impute: per-marker CSV to write (missing, imputed, no_donor, undecided, neighbours)")
    from .tag_impute import add_tuning
    add_tuning(ap.add_argument_group("--impute (its LD shares --ld-min-shared)"), prefix="impute-", min_r2="--impute-min-r2", ld_min_shared=False)
    ap.add_argument("--parentage", metavar="FILE", help="parentage CSV to write: the samples' parent pairs over the markers that pass (see tag_parentage)")
    ap.add_argument("--parentage-offspring", metavar="FILE", help="--parentage: names of the samples to find parents for, one per line (default: all)")
    ap.add_argument("--parentage-parents", metavar="FILE", help="--parentage: names of the samples that may be parents, one per line (default: all)")
    ap.add_argument("--parentage-trios", metavar="FILE", help="--parentage: trios CSV to write (one row per ranked trio)")
    ap.add_argument("--rule", choices=list(tf.GENO_RULES), default="likelihood",
                    help="likelihood: heterozygous when the rarer allele's reads are too many for errors; presence: when both were seen")
    ap.add_argument("--err", type=float, default=0.01, help="sequencing error rate of the likelihood rule")
    ap.add_argument("--min-depth", type=int, default=1, help="fewer reads of both tags together: missing")
    ap.add_argument("--min-call-rate", type=float, default=0.0, help="drop markers called in a smaller share of the samples")
    ap.add_argument("--min-maf", type=float, default=0.0, help="drop markers with a smaller minor allele frequency")
    ap.add_argument("--max-het", type=float, default=1.0, help="drop markers with a larger share of heterozygous calls")
    ap.add_argument("--td-device", type=int, default=0, help="GPU to run on")
    ap.add_argument("--td-backend", choices=["gpu", "host"], default="gpu", help="host: numpy on the CPU (with -i)")
    return ap


def add_vcf_options(ap, likelihoods):
    ap.add_argument("--vcf", metavar="FILE", help="VCF file to write (markers that pass; GT:AD:DP per sample)")
    if likelihoods:
        ap.add_argument("--vcf-likelihoods", action="store_true", help="--vcf: add GQ:PL from the error rate --err")
    ap.add_argument("--vcf-positions", metavar="names|FILE",
                    help="--vcf: CHROM and POS from marker names chrom-pos-strand (names) or from a CSV: Marker name, Chromosome, Position")


def read_positions(spec):
    """What writeVCF takes as positions: None, "names", or the dict of a CSV with a header row."""
    if spec is None or spec == "names":
        return spec
    where = {}
    with open(spec, newline="") as fh:
        rows = csv.reader(fh)
        next(rows, None)
        for row in rows:
            if row:
                if len(row) < 3 or not row[2].strip().isdigit():
                    raise Exception("{}: expected Marker name, Chromosome, Position in every row, found {}.".format(spec, row))
                where[row[0]] = (row[1], int(row[2]))
    return where


def read_counts(path):
    """(sample names, tag names, uint32 matrix) of a CSV written by writeCounts."""
    import numpy as np
    from .engine import counts_as_uint32
    with open(path, newline="") as fh:
        rows = csv.reader(fh)
        header = next(rows, None)
        if header is None or len(header) < 2 or header[0] != "":
            raise Exception("{}: not a counts file (an empty first header cell, then tag names, expected).".format(path))
        samples, data = [], []
        for row in rows:
            if row:
                if len(row) != len(header):
                    raise Exception("{}: sample {} has {} counts, the header names {} tags.".format(
                        path, row[0], len(row) - 1, len(header) - 1))
                samples.append(row[0])
                data.append([int(x) for x in row[1:]])
    matrix = np.array(data, dtype=np.uint64).reshape(len(samples), len(header) - 1)
    return samples, header[1:], counts_as_uint32(matrix)


def read_tags(args):
    """[tag names, tag sequences] by the one tag format whose options were given, prefix-free (sanitizeTags)."""
    keep = checked(tf.readMarkerNames(args.tokeep), "marker names to keep") if args.tokeep is not None else None
    tags = checked(TAG_FORMATS[tag_format(args)][1](args, keep, args.binaryOnly == "T"), "tags")
    return tf.sanitizeTags(tags)


def count_on_device(eng, keys, sequences, site, maxreads):
    """Every library of the key file counted and folded into one samples x tags uint32 matrix in device memory
    (combineReadCounts' sample order).  Returns (sample names, DeviceCounts); the buffer is the caller's."""
    samples, rows = tf.sample_rows(keys)
    nbytes = len(samples) * len(sequences) * 4
    d_total = eng.dev_alloc(nbytes)
    try:
        zeros = bytes(min(nbytes, 64 << 20))
        for off in range(0, nbytes, len(zeros) or 1):
            eng.h2d(d_total + off, zeros[:nbytes - off])
        eng.set_option("progress", 0)
        for f in sorted(keys):
            eng.set_index(keys[f][0], sequences, site)
            eng.count_file(f, maxreads)
            eng.fold_rows(rows[f], d_total, len(samples))
    except BaseException:
        eng.dev_free(d_total)
        raise
    return samples, tf.DeviceCounts(d_total, (len(samples), len(sequences)))


def stats_line(result):
    missing = int((result.calls == tf.GENO_MISSING).sum())
    return "Samples: {} Markers: {} Passed: {} Calls: {} Missing: {}".format(
        len(result.samples), len(result.markers), result.stats["passed"], result.calls.size - missing, missing)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if (args.counts is None) == (args.barcodefile is None):
        raise Exception("Need either a counts file (-i) or a key file whose libraries are counted (-b, tags and -e or -c).")
    have_tags = any(getattr(args, o) is not None for o in FILE_OPTIONS)
    if args.hapmap is not None and not have_tags:
        raise Exception("--hapmap needs the tag file (e.g. --MergedTags) for the alleles' bases.")
    params = dict(rule=args.rule, err=args.err, min_depth=args.min_depth, min_call_rate=args.min_call_rate,
                  min_maf=args.min_maf, max_het=args.max_het, device=args.td_device)
    relate = args.relations is not None or args.relations_matrix is not None
    if args.relations_ld_pruned and not relate:
        raise Exception("--relations-ld-pruned goes with --relations or --relations-matrix.")
    ld = args.relations_ld_pruned or any(x is not None for x in (args.ld, args.ld_groups, args.ld_keep))
    if args.impute_stats is not None and args.impute is None:
        raise Exception("--impute-stats goes with --impute.")
    impute = args.impute is not None
    if args.parentage is None and any(x is not None for x in (args.parentage_offspring, args.parentage_parents, args.parentage_trios)):
        raise Exception("--parentage-offspring, --parentage-parents and --parentage-trios go with --parentage.")
    parent = args.parentage is not None
    if args.vcf is None and (args.vcf_likelihoods or args.vcf_positions is not None):
        raise Exception("--vcf-likelihoods and --vcf-positions go with --vcf.")
    positions = read_positions(args.vcf_positions)
    eng = d_counts = d_calls = relations = ldres = ld_keep = imputed = parents = None
    if args.counts is not None:
        if args.counts_out is not None:
            raise Exception("--counts-out goes with counting (-b); -i is that file already.")
        samples, names, counts = read_counts(args.counts)
        sequences = None
        if have_tags:
            tagnames, tagseqs = read_tags(args)
            where = {n: k for k, n in enumerate(tagnames)}
            missing = [n for n in names if n not in where]
            if missing:
                raise Exception("Tag {} of the counts file is not in the tag file.".format(missing[0]))
            sequences = [tagseqs[where[n]] for n in names]
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
        # relations, LD, imputation, parentage and the VCF writer read the calls where the call kernel wrote them
        keep = (relate or ld or impute or parent or args.vcf is not None) and backend == "gpu"
        result = tf.call_genotypes(counts, samples, names, backend=backend, keep_device=keep, **params)
        d_calls = result.d_calls
        if d_counts is not None and args.counts_out is not None:
            import numpy as np
            host = np.frombuffer(eng.d2h(d_counts.ptr, d_counts.shape[0] * d_counts.shape[1] * 4), dtype=np.uint32)
            tf.writeCounts(args.counts_out, host.reshape(d_counts.shape), samples, names)
        if args.vcf is not None:                         # (while the matrix and the calls are on the device)
            tf.writeVCF(args.vcf, result, counts, tagseqs=sequences, positions=positions, passing_only=True,
                        likelihoods=args.vcf_likelihoods, err=args.err, device=args.td_device, backend=backend)
        if ld:
            ldres = tf.marker_ld(d_calls if keep else result.calls, result.markers, mask=result.mask, min_r2=args.min_r2,
                                 min_shared=args.ld_min_shared, device=args.td_device, backend=backend)
            ld_keep = tf.ld_prune(ldres)
        if relate:
            relations = tf.sample_relations(d_calls if keep else result.calls, samples,
                                            mask=result.mask & ld_keep if args.relations_ld_pruned else result.mask, max_dist=args.max_dist,
                                            min_shared=args.min_shared, device=args.td_device, backend=backend)
        if parent:
            from .tag_parentage import read_names
            parents = tf.parentage(d_calls if keep else result.calls, samples, offspring=read_names(args.parentage_offspring),
                                   parents=read_names(args.parentage_parents), mask=result.mask, device=args.td_device, backend=backend)
        if impute:
            from .tag_impute import tuning
            imputed = tf.impute_calls(d_calls if keep else result.calls, result.markers, mask=result.mask, device=args.td_device,
                                      backend=backend, **tuning(args))
            if keep:                                     # the filled matrix comes to the host once, to be written
                import numpy as np
                dev, filled, (S, M) = tf.default_engine(args.td_device), imputed.calls, imputed.calls.shape
                try:
                    imputed.calls = np.frombuffer(dev.d2h(filled.ptr, S * M) if filled.ptr else b"", dtype=np.uint8).reshape(S, M)
                finally:
                    if filled.ptr:
                        dev.dev_free(filled.ptr)
    finally:
        if d_counts is not None:
            eng.dev_free(d_counts.ptr)
        if d_calls is not None and d_calls.ptr:
            tf.default_engine(args.td_device).dev_free(d_calls.ptr)
    tf.writeGenoCalls(args.output, result, passing_only=True)
    if args.stats is not None:
        tf.writeMarkerStats(args.stats, result)
    if args.hapmap is not None:
        tf.writeHapMap(args.hapmap, result, sequences, passing_only=True)
    if args.relations is not None:
        tf.writeRelations(args.relations, relations)
    if args.relations_matrix is not None:
        tf.writeDistanceMatrix(args.relations_matrix, relations)
    if args.ld is not None:
        tf.writeLDPairs(args.ld, ldres)
    if args.ld_groups is not None:
        tf.writeLDGroups(args.ld_groups, ldres, keep=ld_keep)
    if args.ld_keep is not None:
        from .tag_ld import write_keep
        write_keep(args.ld_keep, ldres, ld_keep)
    if impute:
        tf.writeGenoCalls(args.impute, tf.GenoResult(result.markers, result.samples, imputed.calls, result.stats, result.mask,
                                                     result.columns), passing_only=True)
        if args.impute_stats is not None:
            tf.writeImputeStats(args.impute_stats, imputed)
    if parent:
        tf.writeParentage(args.parentage, parents)
        if args.parentage_trios is not None:
            tf.writeTrios(args.parentage_trios, parents)
    print(stats_line(result))
    if impute:
        from .tag_impute import summary_line
        print(summary_line(imputed))
    if parent:
        from .tag_parentage import summary_line as parentage_line
        print(parentage_line(parents))
    return 0


if __name__ == "__main__":
    sys.exit(main())
