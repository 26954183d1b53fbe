"""The solve spec of the loss, mask and weight entry points (tscm_calib_amd/csrc/tscm_spec.h), checked by
tests/native/spec_check.cpp: every single fault of make_spec and check_corner_weights comes back with its code and text, the
loss constants are Ceres' (b = a^2, c = 1 / b), and scatter_weights agrees with a brute-force loop on random ragged problems in
a solver's layout (a permuted subset of the views) and in a batch's slot order (problems with and without weights).
Built twice: plain, and under AddressSanitizer + UBSan.  No GPU."""
import pytest

from tests import native_check as N

E_INVALID = -1
LOSS_KIND = "unknown loss kind"
LOSS_SCALE = "the scale of a loss must be finite and > 0"
MASK = "unknown bits in a fixed-intrinsics mask (bits 0-8 only)"

pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("spec_check.cpp", "spec_check")


def test_header_is_plain_cpp17():
    N.assert_plain_cpp17("tscm_spec.h")


def test_refusals(checker):
    r = N.run(checker, "refusals")
    assert r == {
        "ok": True, "why": "",
        "ok_none": [0, ""], "ok_none_any_scale": [0, ""], "ok_cauchy": [0, ""],
        "kind_low": [E_INVALID, LOSS_KIND], "kind_high": [E_INVALID, LOSS_KIND],
        "scale_zero": [E_INVALID, LOSS_SCALE], "scale_negative": [E_INVALID, LOSS_SCALE],
        "scale_nan": [E_INVALID, LOSS_SCALE], "scale_inf": [E_INVALID, LOSS_SCALE],
        "mask_bits": [E_INVALID, MASK], "mask_bits_beyond_n": [0, ""],
        # views of 3, 0, 2 and 4 corners: corner n, view v and corner j of the view
        "w_ok": [0, ""],
        "w_negative": [E_INVALID, "corner weight 6 (view 3, corner 1) is negative, NaN or infinite"],
        "w_nan": [E_INVALID, "corner weight 4 (view 2, corner 1) is negative, NaN or infinite"],
        "w_inf": [E_INVALID, "corner weight 2 (view 0, corner 2) is negative, NaN or infinite"],
        "w_view_all_zero": [E_INVALID, "every corner weight of view 2 is 0: pass view_count = 0 for a view without corners"],
    }


def test_loss_constants(checker):
    r = N.run(checker, "loss")
    assert r["ok"], r


@pytest.mark.parametrize("seed", [1, 2])
def test_scatter_weights_against_brute_force(checker, seed):
    r = N.run(checker, "scatter", seed, 300)
    assert r["ok"], r
    # what the sample must have exercised
    assert r["empty_views"] > 0 and r["subsets"] > 0 and r["masked_nan"] > 0 and r["unweighted"] > 0, r
