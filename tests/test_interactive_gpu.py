"""Whole sessions of the interactive front-ends on an MI355X against sessions recorded from the reference
(tests/golden/interactive.json): two input files of eight barcodes split with adapter read-through, MD5 sums asked for
and not; Merged and UNEAK tags counted in a 60 000-read file (a progress line appears) and a small one, genotypes asked
for and not.  Stdout and every file written -- the split FASTQ files, the MD5 CSV, counts and genotypes -- byte for
byte.  The MD5 session is also run with the device threshold of writeMD5sums at 1, so that its sums come from the GPU."""
import os
import subprocess
import sys

import pytest

import interactive_cases as ic

pytestmark = pytest.mark.gpu
GOLDEN = {t["name"]: t for t in ic.load("interactive.json")["transcripts"]}
CASES = [c for c in ic.transcripts() if c["gpu"]]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_transcript(case, tmp_path):
    ic.run_transcript(case, GOLDEN[case["name"]], tmp_path)


def test_splitter_md5_host_backend(tmp_path):
    case = next(c for c in CASES if c["name"] == "split_two_files_md5_yes")
    ic.run_transcript(case, GOLDEN[case["name"]], tmp_path, ["--td-backend", "host"])


def test_splitter_md5_on_the_device(tmp_path):
    """The session with MD5 sums, the 16 output files hashed by td_md5_files (the threshold lowered in the child)."""
    case = next(c for c in CASES if c["name"] == "split_two_files_md5_yes")
    golden = GOLDEN[case["name"]]
    d = os.path.realpath(str(tmp_path))
    ic.write_files(d, case["files"])
    code = ("import sys\nfrom tagdigger_amd import tagdigger_fun as tf, barcode_splitter, engine\n"
            "tf._MD5_DEVICE_MIN_FILES = 1\nreal = engine.Engine.md5_files\n"
            "def spy(self, paths):\n    sys.stderr.write('device md5: %d files\\n' % len(paths))\n    return real(self, paths)\n"
            "engine.Engine.md5_files = spy\nsys.exit(barcode_splitter.main([]))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=d, input=case["stdin"].encode(), capture_output=True,
                       env=ic.child_env(), timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert "device md5: 16 files" in r.stderr.decode()
    assert r.stdout.decode().replace(d, "{CWD}").split("Press enter to begin")[1] == \
        ic.unpack(golden["stdout_b64"]).decode().split("Press enter to begin")[1]
    for name, b64 in golden["outputs"].items():
        assert open(os.path.join(d, name), "rb").read() == ic.unpack(b64), name
