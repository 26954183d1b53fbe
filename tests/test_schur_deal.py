"""k_schur_gram's deal of a chunk's board groups over the four waves of its workgroup (tscm_calib_amd/csrc/tscm_layout.h:
schur_group_of, schur_virtual_wave), checked by tests/native/schur_deal_check.cpp for every chunk size 1..64
and every rot 0..3: each group of four boards is taken exactly once, the waves' counts differ by at most one, the
(virtual wave, k) -> group map does not depend on rot, and 64 boards are 4/4/4/4.  Built twice: plain, and under
AddressSanitizer + UBSan.  No GPU."""
from tests import native_check as N

pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("schur_deal_check.cpp", "schur_deal_check")


def test_header_is_plain_cpp17():
    N.assert_plain_cpp17("tscm_layout.h")


def test_every_group_once_and_evenly_for_every_chunk_size_and_rot(checker):
    r = N.run(checker, "deal")
    assert r["ok"], r
    assert r["cases"] == 64 * 4
    assert r["boards64"] == [4, 4, 4, 4]
    assert r["boards40"] == [3, 3, 2, 2]          # config 4's chunks: was 4, 4, 2, 0
    assert r["boards16"] == [1, 1, 1, 1] and r["boards17"] == [2, 1, 1, 1]


def test_chunks_mode_reports_plan_layouts_chunks(checker):
    """100 boards seen by cameras 0 and 1, then 21 seen by camera 1 alone, on 2 CUs: chunks of ceil(121 / 4) = 31 boards per
    signature, the one-view boards first (the GPU test of the deal takes its board counts from this mode)."""
    views = [(c, b, 6) for b in range(100) for c in (0, 1)] + [(1, 100 + b, 6) for b in range(21)]
    words = [2, 121, 6, len(views), *[x for v in views for x in v], 2, 16]
    r = N.run(checker, "chunks", stdin=" ".join(map(str, words)))
    assert r == {"slow_boards": 0, "chunks": [[1, 21], [2, 31], [2, 31], [2, 31], [2, 7]]}
