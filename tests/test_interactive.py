"""The interactive front-ends (python -m tagdigger_amd.barcode_splitter, python -m tagdigger_amd.tagdigger_interactive)
against sessions recorded from the reference's barcode_splitter.py and tagdigger_interactive.py
(tests/golden/interactive.json): the sessions that end before any file is processed -- stdin runs out at a prompt,
wrong answers at every loop, the unreadable-FASTQ menu with its three choices, key files that do not parse.  No GPU."""
import pytest

import interactive_cases as ic

GOLDEN = {t["name"]: t for t in ic.load("interactive.json")["transcripts"]}
CASES = [c for c in ic.transcripts() if not c["gpu"]]


def test_golden_covers_the_cases_defined():
    assert sorted(GOLDEN) == sorted(c["name"] for c in ic.transcripts())
    for c in ic.transcripts():
        assert GOLDEN[c["name"]]["program"] == c["program"] and GOLDEN[c["name"]]["gpu"] == c["gpu"]
    # the early endings are the reference's EOFError after a prompt; the whole sessions end normally
    assert all(GOLDEN[c["name"]]["exception"] == "EOFError: EOF when reading a line" for c in CASES)
    assert all(GOLDEN[c["name"]]["returncode"] == 0 for c in ic.transcripts() if c["gpu"])
    assert {c["program"] for c in CASES} == set(ic.PROGRAMS)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_transcript(case, tmp_path):
    ic.run_transcript(case, GOLDEN[case["name"]], tmp_path)


def test_options_of_this_build():
    from tagdigger_amd import barcode_splitter, tagdigger_interactive
    a = barcode_splitter.build_parser().parse_args(["--td-device", "3", "--td-backend", "host"])
    assert (a.td_device, a.td_backend) == (3, "host")
    assert barcode_splitter.build_parser().parse_args([]).td_backend == "gpu"
    assert tagdigger_interactive.build_parser().parse_args(["--td-device", "2"]).td_device == 2
