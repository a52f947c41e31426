#!/usr/bin/env python3
"""Generate tests/golden/interactive.json and tests/golden/md5sums.json from the REAL reference (build container only;
data only, never reference code).  The cases and their input files are defined in tests/interactive_cases.py.

  interactive.json  barcode_splitter.py and tagdigger_interactive.py run in a scratch directory holding the case's
                    files, its answers piped on stdin: stdout (the scratch directory's path replaced by {CWD}), every
                    file written or changed, the exception's last traceback line (or null), and the MD5 sums of the
                    input files (they are rebuilt from seeds by the tests);
                    remove_monomorphic_loci of the reference module called directly.
  md5sums.json      writeMD5sums of the reference module: the input files, the CSV it wrote, stdout, the exception.
Payloads are base64 of a zlib stream.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_interactive_golden.py REFERENCE_DIR
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import interactive_cases as ic  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else None


def run_transcript(c):
    with tempfile.TemporaryDirectory() as d:
        d = os.path.realpath(d)
        ic.write_files(d, c["files"])
        before = ic.snapshot(d)
        env = dict(os.environ, PYTHONHASHSEED="0", PYTHONDONTWRITEBYTECODE="1")
        r = subprocess.run([sys.executable, os.path.join(REF, c["program"] + ".py")], cwd=d, input=c["stdin"].encode(),
                           capture_output=True, env=env, timeout=900)
        outputs = {k: ic.pack(v) for k, v in ic.snapshot(d).items() if before.get(k) != v}
        err = r.stderr.decode().strip().splitlines()
        return {"name": c["name"], "program": c["program"], "gpu": c["gpu"],
                "inputs_md5": {k: hashlib.md5(v).hexdigest() for k, v in c["files"].items()},
                "stdout_b64": ic.pack(r.stdout.decode().replace(d, "{CWD}")), "returncode": r.returncode,
                "exception": err[-1] if r.returncode else None, "outputs": outputs}


def run_md5(ref, c):
    with tempfile.TemporaryDirectory() as d:
        ic.write_files(d, c["files"])
        old = os.getcwd()
        os.chdir(d)
        try:
            rec = ic.call_recorded(ref.writeMD5sums, [c["filelist"], "md5_out.csv"])
            rec.pop("result", None)
            rec["csv_b64"] = ic.pack(open("md5_out.csv", "rb").read()) if os.path.exists("md5_out.csv") else None
        finally:
            os.chdir(old)
    rec.update(name=c["name"], filelist=c["filelist"], files={k: ic.pack(v) for k, v in c["files"].items()})
    return rec


def dump(path, data):
    with open(path, "w") as fh:                         # one record per line
        fh.write("{\n")
        for k, key in enumerate(sorted(data)):
            fh.write('"%s": [\n%s\n]' % (key, ",\n".join(json.dumps(v, sort_keys=True) for v in data[key])))
            fh.write(",\n" if k + 1 < len(data) else "\n}\n")
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


def main():
    sys.path.insert(0, REF)
    import tagdigger_fun as ref
    ts = [run_transcript(c) for c in ic.transcripts()]
    mono = []
    for names, seqs, verbose in ic.MONO_CASES:
        rec = ic.call_recorded(ref.remove_monomorphic_loci, [names, seqs], {"verbose": verbose})
        rec["args"] = [names, seqs, verbose]
        mono.append(rec)
    dump(os.path.join(HERE, "interactive.json"), {"transcripts": ts, "remove_monomorphic_loci": mono})
    dump(os.path.join(HERE, "md5sums.json"), {"cases": [run_md5(ref, c) for c in ic.md5_cases()]})
    for t in ts:
        print("  %-36s rc=%d %s" % (t["name"], t["returncode"], t["exception"] or ""))


if __name__ == "__main__":
    if not REF:
        sys.exit(__doc__)
    main()
