"""inference.py / validate.py with --cascade_dirs on TFRecord files at the small dims of test_gpu_ensemble_inference.py: one trained
checkpoint plus its converted student, built once per module in one child process (tests/_cascade_child.py, under EVC_DETERMINISTIC=1),
at --precision bf16, 16 videos in batches of 5, 5, 5, 1.

Every file is compared line by line, with ==, with tests/_cascade_ref.py applied to the towers' own EvalGraph predictions on the same
batches.  That rests on a bf16 tower's row not depending on which other rows of the batch are live: each row's MFMA products and K order
are its own, and ops.RowPlan moves rows between slots, not values between rows.  validate's numbers are compared with eval_util on the
reference's merged predictions (== except the loss: the device sums 4716 f32 terms of one sign per row, 4716 * 2^-24 relative bounds every
order of such a sum).  --precision high is not bit-stable under a changing live set (its MoE head takes its e4m3 range from the batch's
max|x|): one case runs there and is held to the float64 oracle of the tower that decided each video, 1e-3 + 1e-6, the bound of
test_gpu_inference.py for one tower."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORACLE_BOUND = 1e-3 + 1e-6
LOSS_REL = 4716 * 2.0 ** -24


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    work = tmp_path_factory.mktemp("cascade")
    result = work / "result.pkl"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_cascade_child.py"), str(work), str(result)],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(result, "rb") as f:
        return pickle.load(f)


def _check_case(case, towers, stage_videos=None):
    st = case["stats"]
    assert st["tower"] == "cascade" and st["videos"] == 16 and st["batches"] == 4
    assert [(t, e) for _, t, e in st["members"]] == towers
    assert len(case["lines"]) == len(case["expected"]) == 16
    for got, exp in zip(case["lines"], case["expected"]):
        assert got == exp
    assert st["stage_videos"] == case["expected_rows"]
    if stage_videos is not None:
        assert st["stage_videos"] == stage_videos
    assert st["stage_videos"][0] == 16 and st["gate_wait_s"] >= 0.0 and len(st["stage_frames"]) == len(towers)
    return st


TWO = [("student", 30), ("teacher", 1)]


def test_a_threshold_minus_inf_is_the_student_alone(child):
    """Nobody escalates: the student's file, and the teacher's graph is never stepped."""
    st = _check_case(child["cases"]["a"], TWO, [16, 0])
    assert child["cases"]["a"]["lines"] == child["cases"]["single_student30"]["lines"]
    assert st["stage_steps"] == [4, 0] and st["stage_frames"][1] == 0 and st["stage_frames"][0] > 0


def test_b_fraction_one_is_the_teacher_alone(child):
    st = _check_case(child["cases"]["b"], TWO, [16, 16])
    assert child["cases"]["b"]["lines"] == child["cases"]["single_teacher"]["lines"]
    assert child["cases"]["b"]["lines"] != child["cases"]["single_student30"]["lines"]
    assert st["stage_steps"] == [4, 4] and st["stage_frames"][1] > st["stage_frames"][0]         # the teacher reads ~30 times the frames


def test_c_median_threshold_serves_each_video_from_the_tower_that_decided_it(child):
    decided = child["c_decided"]
    assert 0 < sum(decided.values()) < 16, "the median threshold left a stage without a video: change the data seed"
    case = child["cases"]["c"]
    st = _check_case(case, TWO)
    assert st["stage_videos"] == [16, sum(decided.values())]
    for line in case["lines"]:
        vid = line.split(",")[0]
        assert line == child["c_single"][(("student30", "teacher")[decided[vid]], vid)]
    assert case["lines"] != child["cases"]["a"]["lines"] and case["lines"] != child["cases"]["b"]["lines"]


def test_d_margin_with_half_of_each_batch(child):
    st = _check_case(child["cases"]["d"], TWO)
    assert st["stage_videos"][1] == 3 + 3 + 3 + 1                                            # ceil(0.5 * 5) per batch of 5, ceil(0.5 * 1) for the last


def test_e_three_stages_and_the_stage_file(child):
    st = _check_case(child["cases"]["e"], [("student", 30), ("student", 10), ("teacher", 1)])
    dirs = [d for d, _, _ in st["members"]]
    assert dirs[0] == dirs[1] != dirs[2]
    assert st["stage_videos"][1] <= 3 + 3 + 3 + 1 and st["stage_videos"][2] <= st["stage_videos"][1]      # ceil(0.6 * 5) = 3, ceil(0.6 * 1) = 1
    assert st["stage_videos"][1] > 0, "nobody left the first stage: change the data seed"
    assert child["e_stage_file"] == child["e_stage_expected"]
    assert child["e_stage_file"].count("\n") == 17


def test_f_validate_evaluates_the_merged_predictions(child):
    host, device, want = child["validate_host"], child["validate_device"], child["validate_expected"]
    assert child["ties_at_k"] == [] and child["ties_at_n_pos"] == [], "rows with an exact tie at a selection boundary: change the data seed"
    for name, got in (("host", host), ("device", device)):
        assert got is not None and "student_loss" not in got
        for key in ("avg_hit_at_one", "avg_perr", "gap"):
            print(name, key, got[key], want[key])
            assert got[key] == want[key], (name, key)
        assert np.array_equal(np.asarray(got["aps"]), np.asarray(want["aps"])), name
        print(name, "avg_loss", got["avg_loss"], want["avg_loss"])
        assert abs(got["avg_loss"] - want["avg_loss"]) <= LOSS_REL * abs(want["avg_loss"]), name
        assert got["cascade_stage_videos"] == child["validate_expected_rows"]
    assert want["gap"] > 0 and want["avg_loss"] > 0
    for key in ("avg_hit_at_one", "avg_perr", "gap", "avg_loss", "epoch_id", "cascade_stage_videos", "cascade_stage_frames"):
        assert host[key] == device[key], key
    assert np.array_equal(np.asarray(host["aps"]), np.asarray(device["aps"]))


def test_precision_high_stays_within_the_oracle_bound(child):
    high = child["high"]
    assert high["videos"] == 16 and high["stats"]["stage_videos"][0] == 16
    assert set(high["decided"].values()) <= {0, 1} and sum(high["decided"].values()) == high["stats"]["stage_videos"][1]
    print("worst distance from the float64 oracle of the deciding tower: %.3e" % high["worst"])
    assert high["worst"] < ORACLE_BOUND
