"""Host logic of a solve's launch sequence (tscm_calib_amd/csrc/tscm_exec_plan.h: plan_exec, check_exec_options), checked by
tests/native/exec_plan_check.cpp: the rows of DESIGN 4's launch table as decisions; on random problems under random and
boundary residency figures, that a re-run never waits inside a launch, that every launch whose workgroups wait for each other
fits on the chip and that each exec flag changes only what it names; and the option refusals.  Built twice: plain, and under
AddressSanitizer + UBSan.  No GPU."""
import pytest

from tests import native_check as N

E_INVALID, E_UNSUPPORTED = -1, -5
ITERATIONS = "max_num_iterations must be in [0, 255]"
UNKNOWN_BITS = "unknown bits in tscm_options.exec_flags (an options struct of an older ABI?)"
NO_ROBUST = "TSCM_EXEC_GRAM_16X16 has no robust-loss kernel"

pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("exec_plan_check.cpp", "exec_plan_check")


def test_header_is_plain_cpp17():
    N.assert_plain_cpp17("tscm_exec_plan.h")


def test_design_table_rows(checker):
    r = N.run(checker, "rows")
    # config 4 (one GPU, 4 cameras, every board seen by two): k_schur_gram<2, true> with the reductions riding ->
    # k_solve_reduced<4, 16, 64, true> with the T producers and every back-substitution workgroup -> the Gram kernel
    c4 = r["config4"]
    assert c4["launches"] == 3 and c4["tail"] == "ride" and c4["stats_ride"] and c4["ctl_in_schur"], c4
    assert c4["solver"] == "dense4" and c4["t_in_solve"] and c4["n_prod"] > 0, c4
    assert c4["n_bs"] == c4["n_bs_blocks"] > 0 and c4["bs_threads"] == 0 and not c4["comm"] and c4["gram"] == 0, c4
    s4 = r["config4_separate_stats"]
    assert s4["launches"] == 4 and s4["tail"] == "stats_head" and not s4["stats_ride"] and s4["ctl_in_schur"], s4
    # a one-rank communicator is the one-GPU path unless TSCM_EXEC_KEEP_SINGLE_RANK_COMM asks for the communicator's
    assert r["config4_one_rank_comm"] == c4
    assert r["config4_keep_one_rank_comm"] == r["config4_comm"]
    # the communicator (<= 8 cameras): k_schur_gram (the step on the all-reduced H_stage) -> k_T_reduce -> solve launch with the
    # back-substitution riding -> Gram kernel -> k_reduce_stats -> k_finalize_eval
    for name in ("config4_comm", "ring8_comm"):
        c = r[name]
        assert c["comm"] and c["tail"] == "exchange" and c["ctl_in_schur"] and not c["stats_ride"], c
        assert not c["t_in_solve"] and c["n_prod"] == 0 and c["n_bs"] == c["n_bs_blocks"] > 0 and c["launches"] == 6, c
    # up to 4 cameras along the camera-pair graph / as one dense block of k_solve_nd
    assert r["config4_graph_order"]["solver"] == "nd" and r["config4_graph_order"]["nd"] == 0
    assert r["config4_dense_order"]["solver"] == "nd" and r["config4_dense_order"]["nd"] == 1
    # 8-camera ring, Schur grid of more than one round: no ride; the back-substitution rides iff all of it fits
    fits, short = r["ring8_bs_fits"], r["ring8_bs_one_short"]
    for c in (fits, short):
        assert c["solver"] == "nd" and not c["stats_ride"] and c["tail"] == "stats_head" and c["t_in_solve"], c
    assert fits["n_bs"] == fits["n_bs_blocks"] > 0 and fits["bs_threads"] == 0 and fits["launches"] == 4, fits
    assert short["n_bs"] == 0 and short["bs_threads"] == 256 and short["launches"] == 5, short
    # 9-32 cameras: k_schur_gram -> k_T_reduce -> k_solve_reduced_big -> k_backsub_prep -> Gram -> k_reduce_stats + k_finalize_eval -> k_control
    rig = r["rig12"]
    assert rig["solver"] == "big" and rig["tail"] == "exchange" and not rig["ctl_in_schur"] and not rig["t_in_solve"], rig
    assert rig["n_bs"] == 0 and rig["bs_threads"] > 0 and rig["launches"] == 8, rig
    # boards seen by more than three cameras: k_schur_factor + k_pair_gram, the control step out of the Schur head
    assert r["slow_boards"] > 0
    for name in ("seen_by_four", "seen_by_four_comm"):
        assert not r[name]["ctl_in_schur"] and not r[name]["stats_ride"], r[name]
    assert r["seen_by_four"]["tail"] == "reduce_control" and r["seen_by_four"]["launches"] == 6
    # no free camera-side column: the empty system, the back-substitution on its own
    e = r["empty"]
    assert e["solver"] == "empty" and not e["t_in_solve"] and e["n_bs"] == 0 and e["bs_threads"] > 0, e


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_problems(checker, seed):
    r = N.run(checker, "random", seed, 200)
    assert r["ok"], r
    # what the sample must have exercised: both rides, each at its boundary, every solver and every flag changing something
    assert r["stats_ride"] > 0 and r["bs_ride"] > 0 and r["bs_limit"] > 0 and r["stats_limit"] > 0, r
    assert r["t_in_solve"] > 0 and r["big"] > 0 and r["empty"] > 0 and r["slow"] > 0, r
    assert all(n > 0 for n in r["flag_changes"]), r


def test_refusals(checker):
    r = N.run(checker, "refusals")
    assert r == {
        "valid": [0, ""],
        "iterations_0": [0, ""],
        "iterations_255": [0, ""],
        "iterations_256": [E_INVALID, ITERATIONS],
        "iterations_negative": [E_INVALID, ITERATIONS],
        "all_flags": [0, ""],
        "flag_256": [E_INVALID, UNKNOWN_BITS],
        "flag_sign_bit": [E_INVALID, UNKNOWN_BITS],
        "gram16_huber": [E_UNSUPPORTED, NO_ROBUST],
        "gram16_soft_l1": [E_UNSUPPORTED, NO_ROBUST],
        "gram16_cauchy": [E_UNSUPPORTED, NO_ROBUST],
        "huber_other_flags": [0, ""],
        "unknown_bits_before_gram16_loss": [E_INVALID, UNKNOWN_BITS],
        "iterations_before_unknown_bits": [E_INVALID, ITERATIONS],
    }
