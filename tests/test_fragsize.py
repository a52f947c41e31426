"""exp_frag_size on the host search backend (no GPU): the whole command line against every golden case recorded from
the reference's exp_frag_size.py -- the CSV's bytes, stdout, or the exception's class and message."""
import pytest

from fragsize_cases import CASES, run_case


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_host_backend(case, tmp_path, monkeypatch, capsys):
    run_case(case, tmp_path, monkeypatch, capsys, ["--td-backend", "host"])


def test_golden_covers_the_contract():
    """The rules the fixtures must exercise are all there (progress lines, both zero divisions, the gzip failures)."""
    names = {c["name"] for c in CASES}
    assert {"many_tags", "empty_cut_site", "empty_cut_site_zero_division", "dir_rename_indexerror", "gz_truncated",
            "gz_bad_crc", "GZ_upper_is_text", "uneak_pairs", "non_ascii_genome", "record_edges"} <= names
    assert any(c["stdout"] for c in CASES)


def test_slice_bounds_match_python():
    """The plan's windows follow slice(a, b).indices(len) for every sign and size."""
    import numpy as np
    from tagdigger_amd.exp_frag_size import _slice_bound
    for length in (0, 1, 5, 3001):
        xs = np.arange(-3010, 3010, dtype=np.int64)
        got = _slice_bound(xs, np.full_like(xs, length))
        want = [slice(int(x), None).indices(length)[0] for x in xs]
        assert got.tolist() == want
