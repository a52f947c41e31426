"""Shared by tests/test_fragsize.py and tests/test_fragsize_gpu.py: the golden cases of tests/golden/fragsize.json
(what the reference exp_frag_size.py did with each set of inputs) and one run of this build's command line over them."""
import base64
import os
import zlib

import pytest

from conftest import load_golden

CASES = load_golden("fragsize.json")


def unpack(b64):
    return zlib.decompress(base64.b64decode(b64))


def class_name(exc):
    cls = type(exc)
    return cls.__qualname__ if cls.__module__ == "builtins" else cls.__module__ + "." + cls.__qualname__


def run_case(case, tmp_path, monkeypatch, capsys, extra):
    """Materialise the case's files, run the command line in their directory, compare with the reference."""
    from tagdigger_amd import exp_frag_size
    for name, b64 in case["files"].items():
        p = tmp_path / name
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(unpack(b64))
    monkeypatch.chdir(tmp_path)
    args = case["args"]
    wd = args[args.index("-w") + 1] if "-w" in args else "."
    out = os.path.join(str(tmp_path), wd, args[args.index("-o") + 1] if "-o" in args else "out.csv")
    capsys.readouterr()
    if case["exception"]:
        with pytest.raises(BaseException) as ei:
            exp_frag_size.main(args + extra)
        assert class_name(ei.value) == case["exception"]["class"]
        want = case["exception"]["message"]
        # (the traceback printer appends its "Did you mean" hint to a NameError's message)
        assert str(ei.value) == want or want.startswith(str(ei.value) + ". Did you mean")
        assert not os.path.exists(out), "a CSV was written although the run raised"
    else:
        exp_frag_size.main(args + extra)
        with open(out, "rb") as fh:
            assert fh.read() == unpack(case["csv_b64"])
    assert capsys.readouterr().out == case["stdout"]
