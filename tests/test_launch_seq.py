"""Host logic of the LM loop's launch sequence (tscm_calib_amd/csrc/tscm_launch_seq.h: seq_begin, seq_iteration, seq_finish,
ctrl_head_from_options), checked by tests/native/launch_seq_check.cpp: the kernels of each phase of a solve for DESIGN 4's
configurations; whole solves of 0, 1, 2 and K iterations on random problems under random and boundary residency figures,
replayed against a model of the device's hand-off counters (riding reductions, control epochs, riding solve epochs), with
one control step per evaluation, no reductions dropped at the end, every waiting launch resident, a re-run without waiting
launches, the fault injection on exactly the launches it names and the exchange markers where DESIGN 4 puts them; and the
control block's head.  Built twice: plain, and under AddressSanitizer + UBSan.  No GPU."""
import pytest

from tests import native_check as N


pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("launch_seq_check.cpp", "launch_seq_check")


@pytest.mark.parametrize("header", ["tscm_launch_seq.h", "tscm_ctrl.h"])
def test_header_is_plain_cpp17(header):
    N.assert_plain_cpp17(header)


def test_design_table_sequences(checker):
    r = N.run(checker, "rows")
    assert r.pop("ok"), r["failed"]
    r.pop("failed")
    # config 4: the initial evaluation's step in the first Schur head, the candidates' reductions riding in the next one, the
    # last evaluation's reductions and step in the two launches behind the iterations
    c4 = r["config4"]
    assert c4["begin"] == ["begin_view_prep", "eval", "reduce_stats"]
    assert c4["first"] == ["schur2", "solve_dense4_ride", "eval"]
    assert c4["iteration"] == ["schur_ride2", "solve_dense4_ride", "eval"]
    assert c4["finish"] == ["reduce_stats", "finish_solve"]
    s4 = r["config4_separate_stats"]
    assert s4["iteration"] == ["schur2", "solve_dense4_ride", "eval", "reduce_stats"] and s4["finish"] == ["finish_solve"]
    # the re-run after a late hand-off: nothing waits inside a launch
    rr = r["config4_rerun"]
    assert rr["iteration"] == ["schur2", "T_reduce", "solve_dense4", "backsub256", "eval", "reduce_control"]
    assert rr["finish"] == ["end_solve", "copy_ctrl"]
    # the communicator: [all-reduce T] in front of the solve, [all-reduce H_stage] behind k_finalize_eval
    cc = r["config4_comm"]
    assert cc["begin"] == ["begin_view_prep", "eval", "reduce_stats", "finalize_eval", "exchange_H", "control"]
    assert cc["iteration"] == ["schur2", "T_reduce", "exchange_T", "solve_dense4_ride", "eval", "reduce_stats", "finalize_eval", "exchange_H"]
    assert cc["finish"] == ["control", "end_solve", "copy_ctrl"]
    # 8 cameras, a Schur grid of more than one round: no ride; the back-substitution a launch of its own where it does not fit
    assert r["ring8"]["iteration"] == ["schur2", "solve_nd2_ride", "backsub256", "eval", "reduce_stats"]
    # 9-32 cameras
    assert r["rig12"]["iteration"] == ["schur2", "T_reduce", "solve_big", "backsub128", "eval", "reduce_stats", "finalize_eval", "control"]
    assert r["rig12"]["finish"] == ["end_solve", "copy_ctrl"]
    # boards seen by more than three cameras add k_schur_factor + k_pair_gram
    w = r["seen_by_four_comm"]["iteration"]
    assert w[:5] == ["schur_factor", "schur2", "pair_gram", "T_reduce", "exchange_T"] and w[-3:] == ["finalize_eval", "exchange_H", "control"]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_solves(checker, seed):
    r = N.run(checker, "random", seed, 150)
    assert r["ok"], r
    # what the sample must have exercised: both rides, the head's control steps, the end-of-solve reductions of a riding plan,
    # both fault injections, the communicator, 9+ cameras, the re-run options; and the lists stayed within their capacity
    for k in ("schur_ride", "solve_ride", "head_steps", "finish_ride", "withhold_producer", "withhold_stats", "comm", "big", "rerun"):
        assert r[k] > 0, (k, r)
    assert r["max_len"] <= r["capacity"], r


def test_ctrl_head_carries_every_option(checker):
    r = N.run(checker, "head")
    assert r["ok"], r
