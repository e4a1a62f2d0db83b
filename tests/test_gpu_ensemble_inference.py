"""inference.py / validate.py with --ensemble_dirs on TFRecord files at the small dims of test_gpu_inference.py: one trained checkpoint
plus its converted student, built once per module in one child process (tests/_ensemble_child.py, under EVC_DETERMINISTIC=1 so that
two validate runs log the same loss scalar).  Every file is compared line by line with tests/_ensemble_ref.py applied to the members' own
EvalGraph predictions on the same batches, every printed confidence with the float64 oracle combined the same way, and validate's
numbers with eval_util on the host-combined predictions.  No exclusions.

Bounds.  Confidences against the oracle: 1e-3 + 1e-6, the bound of test_gpu_inference.py for one tower at --precision high; it carries
over because max and a convex mean are non-expansive (|max(a, b) - max(a', b')| <= max(|a - a'|, |b - b'|); case (b)'s weights sum to
1) and the f32 weighted sum adds at most M 2^-24 for values in [0, 1].  Loss: the device sums B * 4716 f32 terms per batch, eval_util's
expectation here is float64; V 2^-24 = 2.9e-4 relative is the worst case of an f32 sum of V terms of one sign (the terms are all >= 0),
which bounds every blocked order too.  Everything else is compared with ==."""
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
    work = tmp_path_factory.mktemp("ensemble")
    result = work / "result.pkl"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_ensemble_child.py"), str(work), str(result)],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(result, "rb") as f:
        res = pickle.load(f)
    res["work"] = str(work)
    return res


def _check_case(case, tower, members):
    assert case["stats"]["tower"] == tower and case["stats"]["videos"] == 16 and case["stats"]["batches"] == 4
    assert [(t, e) for _, t, e in case["stats"]["members"]] == members
    assert len(case["lines"]) == len(case["expected"]) == 16
    for got, exp in zip(case["lines"], case["expected"]):
        assert got == exp
    print("worst distance from the float64 oracle: %.3e" % case["worst"])
    assert case["worst"] < ORACLE_BOUND


def test_no_ensemble_flag_writes_the_single_model_file(child):
    """Without an ensemble flag: ops.topk_rows on the one tower, the lines test_gpu_inference.py expects."""
    _check_case(child["cases"]["single_teacher"], "teacher", [("teacher", 10)])
    _check_case(child["cases"]["single_student"], "student", [("student", 10)])


def test_a_teacher_and_converted_student_max(child):
    _check_case(child["cases"]["a"], "ensemble", [("teacher", 10), ("student", 10)])
    assert child["cases"]["a"]["lines"] != child["cases"]["single_teacher"]["lines"]          # the second member is not a spectator
    assert child["cases"]["a"]["lines"] != child["cases"]["single_student"]["lines"]


def test_b_one_directory_twice_and_converted_student_weighted_mean(child):
    case = child["cases"]["b"]
    _check_case(case, "ensemble", [("teacher", 1), ("student", 10), ("student", 10)])
    dirs = [d for d, _, _ in case["stats"]["members"]]
    assert dirs[0] == dirs[1] != dirs[2]


def test_c_teacher_and_the_students_file_max(child):
    case = child["cases"]["c"]
    _check_case(case, "ensemble", [("teacher", 10)])
    assert case["lines"] != child["cases"]["single_teacher"]["lines"]                         # the file's lists change the outcome


def test_validate_evaluates_the_combination(child):
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
    assert want["gap"] > 0 and want["avg_loss"] > 0
    # the two runs: the same numbers, the loss included (fixed-order sum in the child)
    for key in ("avg_hit_at_one", "avg_perr", "gap", "avg_loss", "epoch_id"):
        assert host[key] == device[key], key
    assert np.array_equal(np.asarray(host["aps"]), np.asarray(device["aps"]))
