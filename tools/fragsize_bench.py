#!/usr/bin/env python3
"""exp_frag_size on one MI355X: K1 (genome framing) in GB/s and as a fraction of the 8 TB/s HBM roofline over the bytes
it reads and writes; K2 + K3 (search + gather) in jobs/s; the command line's stage times on a synthetic plain genome
with its tags; and, beside them, the reference's CPU time for the same inputs when its directory is given (else the
issue's measured 125 MB/s of genome, labelled as such).

    python tools/fragsize_bench.py [--gb 3] [--tags 1000000] [--reference DIR]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 8.0


def synth_genome(path, nbytes, nchrom, seed=1):
    """nchrom chromosomes of 60-column ACGT lines, about nbytes in all; returns the chromosome length."""
    rng = np.random.default_rng(seed)
    clen = (nbytes // nchrom) * 60 // 61
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as fh:
        for c in range(nchrom):
            fh.write(b">chr%d\n" % c)
            done = 0
            while done < clen:                     # 60 MB pieces: bounded host memory
                n = min(clen - done, 60 * 1_000_000)
                n -= n % 60 if n >= 60 else 0
                s = alpha[rng.integers(0, 4, n, dtype=np.uint8)]
                rows = s.reshape(-1, 60) if n % 60 == 0 else s.reshape(1, -1)
                fh.write(np.hstack([rows, np.full((rows.shape[0], 1), 10, np.uint8)]).tobytes())
                done += n
    return clen


def synth_sam(path, ntags, nchrom, clen, seed=2):
    rng = np.random.default_rng(seed)
    chrom, pos, flag = rng.integers(0, nchrom, ntags), rng.integers(1, clen, ntags), rng.choice([0, 16], ntags)
    with open(path, "w") as fh:
        fh.write("@HD\tVN:1.0\n")
        fh.writelines("t%d\t%d\tchr%d\t%d\t40\t64M\t*\t0\t0\t%s\t*\n" % (i, flag[i], chrom[i], pos[i], "ACGT" * 16)
                      for i in range(ntags))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gb", type=float, default=3.0, help="genome size in GB (default 3)")
    ap.add_argument("--tags", type=int, default=1_000_000)
    ap.add_argument("--chrom", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reference", help="directory of the reference's exp_frag_size.py: time it on the same inputs")
    ap.add_argument("--tmp", default=None, help="directory for the synthetic files")
    a = ap.parse_args()
    from tagdigger_amd import Engine, exp_frag_size
    from tagdigger_amd.engine import frag_job_dtype
    nbytes = int(a.gb * 1e9)
    with tempfile.TemporaryDirectory(dir=a.tmp) as d:
        fa, sam = os.path.join(d, "genome.fa"), os.path.join(d, "tags.sam")
        t = time.perf_counter()
        clen = synth_genome(fa, nbytes, a.chrom)
        synth_sam(sam, a.tags, a.chrom, clen)
        size = os.path.getsize(fa)
        print("inputs: %.2f GB FASTA (%d x %d bp, 60 columns), %d tags; written in %.1f s" % (
            size / 1e9, a.chrom, clen, a.tags, time.perf_counter() - t))

        eng = Engine(0)
        d_in, d_out = eng.dev_alloc(size + 16), eng.dev_alloc(size + 16)
        eng.load_file_range(fa, 0, size, d_in)
        times = []
        for _ in range(a.reps):
            nout, rows, _, ms = eng.fasta_frame_device(d_in, size, d_out, 64)
            times.append(ms)
        best = min(times)
        traffic = size + nout
        print("K1 k_fasta_summary+scan+emit: %.3f ms best of %d (median %.3f): %.0f GB/s over %.2f GB read + %.2f GB "
              "written = %.1f %% of %.0f TB/s" % (best, a.reps, sorted(times)[len(times) // 2], traffic / best / 1e6,
                                                  size / 1e9, nout / 1e9, 100 * traffic / best / 1e9 / HBM_TBS, HBM_TBS))
        eng.dev_free(d_in)
        rng = np.random.default_rng(3)
        njobs = a.tags
        jobs = np.zeros(njobs, dtype=frag_job_dtype())
        lo = rng.integers(0, nout - 3001, njobs)
        jobs["lo"], jobs["hi"], jobs["tagsize"], jobs["reverse"] = lo, lo + 3001, 64, rng.integers(0, 2, njobs)
        k2 = []
        for _ in range(a.reps):
            out, ms2 = eng.frag_search_device(d_out, nout, jobs, ["CTGCAG", "CCGG"])
            k2.append(ms2)
        found = np.flatnonzero(out[:, 0] >= 0)
        _, ms3 = eng.frag_gather_device(d_out, nout, jobs[found], out[found, 0])
        print("K2 k_frag_search: %d jobs (3 001-byte windows, 2 sites) in %.3f ms = %.1f M jobs/s; K3 k_frag_gather: "
              "%d fragments in %.3f ms; K2 + K3 = %.1f M jobs/s" % (njobs, min(k2), njobs / min(k2) / 1e3, len(found),
                                                                   ms3, njobs / (min(k2) + ms3) / 1e3))
        eng.dev_free(d_out)
        eng.close()

        args = exp_frag_size.build_parser().parse_args(["-s", sam, "-g", fa, "-o", os.path.join(d, "out.csv")])
        t = time.perf_counter()
        with open(os.devnull, "w") as null:
            old, sys.stdout = sys.stdout, null
            try:
                stages, stage_ms = exp_frag_size.run(args)
            finally:
                sys.stdout = old
        wall = time.perf_counter() - t
        print("command line (device path), %.2f GB genome, %d tags: %.2f s wall" % (size / 1e9, a.tags, wall))
        for name, sec in stages:
            print("  %-30s %8.3f s" % (name, sec))
        for k, v in stage_ms.items():
            print("  %-30s %8.3f ms device" % (k, v))
        if a.reference:
            t = time.perf_counter()
            subprocess.run([sys.executable, os.path.join(a.reference, "exp_frag_size.py"), "-s", sam, "-g", fa, "-o",
                            os.path.join(d, "ref.csv")], check=True, stdout=subprocess.DEVNULL,
                           env=dict(os.environ, PYTHONPATH=a.reference))
            ref = time.perf_counter() - t
            print("reference exp_frag_size.py on the same inputs: %.2f s (%.0f MB/s of genome)" % (ref, size / ref / 1e6))
        else:
            print("reference: not run here; its measured rate on a CPU is about 125 MB/s of genome (the issue's figure, "
                  "203 MB FASTA + 20 000 tags in 1.6 s), i.e. about %.0f s for this genome" % (size / 125e6))


if __name__ == "__main__":
    main()
