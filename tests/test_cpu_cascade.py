"""Confidence cascades without a GPU: tests/_cascade_ref.py against a brute-force second statement, every flag refusal of inference.main /
validate.main (before the device is touched), the host bookkeeping of cascade.CascadeGraph (quota, masking, the empty-stage skip, frame
accounting), the stage-file format and the loud CPU-tensor errors of the ops wrappers."""
import math

import numpy as np
import pytest

import _cascade_ref as ref

COMMON = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model",
          "HierarchicalLstmModel", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64", "--every_n", "10"]


@pytest.fixture
def flags():
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


@pytest.fixture
def no_device(monkeypatch):
    """Any device call, checkpoint lookup or record read fails the test."""
    import torch
    from efficientvideoclassification_youtube8m_amd import inference, readers, validate

    def touched(*a, **k):
        raise AssertionError("the device or the data was touched before the flags were checked")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(inference.ops, "check_device", touched)
    monkeypatch.setattr(inference.ops, "cascade_confidence_rows", touched)
    monkeypatch.setattr(inference.ops, "cascade_pick_rows", touched)
    monkeypatch.setattr(readers, "get_input_evaluation_tensors", touched)
    monkeypatch.setattr(inference, "latest_checkpoint", touched)
    monkeypatch.setattr(validate, "latest_checkpoint", touched)


# ---- the reference against a second statement --------------------------------------------------------------------------------------
def _brute_confidence(row, kind):
    vals = [float(v) for v in row]
    if any(math.isnan(v) for v in vals):
        return float("nan")
    s = sorted(vals, reverse=True)
    if kind == "top1":
        return s[0]
    second = s[1] if len(s) > 1 else 0.0
    if math.isinf(s[0]) and s[0] == second:
        return float("nan")
    return float(np.float32(s[0]) - np.float32(second))


def _rows_for_confidence(rng, cols):
    x = ((rng.integers(0, 40, (40, cols)) - 10) / 32.0).astype(np.float32)
    x[3, rng.integers(cols)] = np.nan
    x[4, :] = 0.25
    x[5, rng.integers(cols)] = np.inf
    x[6, :] = np.inf if cols > 1 else 0.5
    x[7, :] = -np.inf if cols > 1 else -0.5
    return x


@pytest.mark.parametrize("cols", [1, 2, 3, 17, 300])
def test_reference_confidence_equals_a_full_sort(cols):
    x = _rows_for_confidence(np.random.default_rng(cols), cols)
    for kind in ("top1", "margin"):
        for row in x:
            got, want = float(ref.confidence(row, kind)), _brute_confidence(row, kind)
            assert (math.isnan(got) and math.isnan(want)) or got == want, (kind, row)


def test_reference_confidence_zero_signs():
    f = lambda *v: np.array(v, np.float32)
    assert np.signbit(ref.confidence(f(-0.0, -1.0), "top1")) and not np.signbit(ref.confidence(f(-0.0, 0.0, -1.0), "top1"))
    assert ref.confidence(f(0.5, 0.5, 0.25), "margin").view(np.uint32) == 0              # two equal maxima: exactly +0
    assert ref.confidence(f(-0.0), "margin").view(np.uint32) == 0x80000000                # one column: -0 - 0.0f
    assert np.isnan(ref.confidence(f(np.inf, np.inf, 1.0), "margin")) and ref.confidence(f(np.inf, 1.0), "margin") == np.inf


def _brute_pick(conf, active, threshold, max_rows):
    rows = len(conf)
    cand = [r for r in range(rows) if (active is None or active[r]) and not (float(conf[r]) >= threshold)]
    if max_rows >= 0:
        cand = [t[2] for t in sorted((math.isnan(float(conf[r])) is False, 0.0 if math.isnan(float(conf[r])) else float(conf[r]), r)
                                     for r in cand)][:max_rows]
    return sorted(cand)


@pytest.mark.parametrize("rows", [1, 7, 200])
@pytest.mark.parametrize("threshold", [-math.inf, math.inf, 0.5, 0.0])
def test_reference_pick_equals_a_full_sort(rows, threshold):
    rng = np.random.default_rng(rows)
    conf = rng.choice(np.array([-0.0, 0.0, 0.25, 0.5, 0.75, np.nan], np.float32), rows)
    nf = rng.integers(1, 301, rows).astype(np.int32)
    active = rng.random(rows) < 0.7
    for act in (None, active):
        n = len(_brute_pick(conf, act, threshold, -1))
        for m in sorted({-1, 0, 1, max(n - 1, 0), n, n + 5}):
            nxt, nfn, count = ref.pick(conf, act, nf, threshold, m)
            want = _brute_pick(conf, act, threshold, m)
            assert np.flatnonzero(nxt).tolist() == want and count == len(want)
            assert np.array_equal(nfn, np.where(nxt != 0, nf, 0)) and nfn.dtype == np.int32 and nxt.dtype == np.uint8
    if threshold == 0.5:                                                                  # AT the threshold: settled
        assert not any(conf[r] == 0.5 for r in _brute_pick(conf, None, threshold, -1))


def test_reference_cascade_loop():
    rng = np.random.default_rng(0)
    b, V = 9, 6
    preds = [rng.random((b, V), dtype=np.float32) for _ in range(3)]
    nf = np.arange(1, b + 1, dtype=np.int32)
    out = ref.cascade(preds, nf, "top1", thresholds=[-np.inf, 0.5])
    assert out["stage_rows"] == [b, 0, 0] and np.array_equal(out["merged"], preds[0]) and not out["stage_of"].any()
    out = ref.cascade(preds, nf, "top1", fractions=[1.0, 1.0])
    assert out["stage_rows"] == [b, b, b] and np.array_equal(out["merged"], preds[2]) and (out["stage_of"] == 2).all()
    out = ref.cascade(preds, nf, "margin", thresholds=[0.3, 0.3], fractions=[0.5, 0.25])
    assert out["stage_rows"][1] <= 5 and out["stage_rows"][2] <= 3
    for r in range(b):
        k = int(out["stage_of"][r])
        assert np.array_equal(out["merged"][r], preds[k][r]) and out["confidence"][r] == ref.confidence(preds[k][r], "margin")
    # a row goes on only from the stage before: the rows of stage 2 are among those of stage 1
    assert set(np.flatnonzero(out["stage_of"] == 2)) <= set(np.flatnonzero(out["stage_of"] >= 1))


# ---- flags -----------------------------------------------------------------------------------------------------------------------
def test_defaults_mean_no_cascade(flags):
    from efficientvideoclassification_youtube8m_amd import inference, validate
    for name in ("dirs", "towers", "every_n", "sampling", "confidence", "thresholds", "fractions", "stage_file"):
        assert getattr(flags, "cascade_" + name) == ""
    assert inference.cascade_spec() is None and inference.ensemble_spec() is None
    assert validate.check_flags() is None


def test_flag_parsing(flags):
    from efficientvideoclassification_youtube8m_amd import inference
    flags.parse(["--cascade_dirs", "s/, s/,t/", "--cascade_towers", "student,student, teacher", "--cascade_every_n", "30, 10,1",
                 "--cascade_sampling", "uniform,last,uniform", "--cascade_confidence", "margin", "--cascade_thresholds=-inf,0.5",
                 "--cascade_fractions", "0.25, 1", "--cascade_stage_file", "stages.csv"])
    spec = inference.cascade_spec()
    assert spec["dirs"] == ["s/", "s/", "t/"] and spec["towers"] == ["student", "student", "teacher"] and spec["every_n"] == [30, 10, 1]
    assert spec["sampling"] == ["uniform", "last", "uniform"] and spec["confidence"] == "margin"
    assert spec["thresholds"] == [-math.inf, 0.5] and spec["fractions"] == [0.25, 1.0] and spec["stage_file"] == "stages.csv"
    flags.reset()
    flags.parse(["--cascade_dirs", "x/,y/", "--every_n", "20", "--cascade_fractions", "0.5", "--student_sampling", "first"])
    spec = inference.cascade_spec()
    assert spec["towers"] == ["auto", "auto"] and spec["every_n"] == [20, 20] and spec["sampling"] == ["first", "first"]
    assert spec["confidence"] == "top1" and spec["thresholds"] is None and spec["fractions"] == [0.5] and spec["stage_file"] == ""


REFUSED = [
    (["--cascade_dirs", "a/,b/", "--cascade_thresholds", "0.5", "--cascade_towers", "teacher"], "cascade_towers"),     # wrong list lengths
    (["--cascade_dirs", "a/,b/", "--cascade_thresholds", "0.5", "--cascade_every_n", "1,2,3"], "cascade_every_n"),
    (["--cascade_dirs", "a/,b/", "--cascade_thresholds", "0.5", "--cascade_sampling", "uniform"], "cascade_sampling"),
    (["--cascade_dirs", "a/,b/", "--cascade_thresholds", "0.5,0.5"], "cascade_thresholds"),
    (["--cascade_dirs", "a/,b/,c/", "--cascade_thresholds", "0.5"], "cascade_thresholds"),
    (["--cascade_dirs", "a/,b/,c/", "--cascade_fractions", "0.5"], "cascade_fractions"),
    (["--cascade_dirs", "a/,b/", "--cascade_thresholds", "0.5", "--cascade_fractions", "0.5,0.5"], "cascade_fractions"),
    (["--cascade_thresholds", "0.5"], "cascade_thresholds"),                                                            # a list for no stages
    (["--cascade_dirs", "a/,b/", "--cascade_fractions", "1.5"], "cascade_fractions"),                                  # outside [0, 1]
    (["--cascade_dirs", "a/,b/", "--cascade_fractions=-0.25"], "cascade_fractions"),
    (["--cascade_dirs", "a/,b/", "--cascade_fractions", "nan"], "cascade_fractions"),
    (["--cascade_dirs", "a/,b/", "--cascade_thresholds", "0.5", "--cascade_confidence", "entropy"], "cascade_confidence"),
    (["--cascade_dirs", "a/,b/", "--cascade_thresholds", "0.5", "--ensemble_dirs", "c/"], "cascade_dirs.*ensemble_dirs"),
    (["--cascade_dirs", "a/,b/", "--cascade_thresholds", "0.5", "--preds_pattern", "x*.csv"], "cascade_dirs.*preds_pattern"),
    (["--cascade_dirs", "a/", "--cascade_fractions", ""], "cascade_dirs"),                                             # fewer than 2 stages
    (["--cascade_dirs", ",".join("d%d/" % i for i in range(9)), "--cascade_fractions", ",".join(["0.5"] * 8)], "cascade_dirs"),
    (["--cascade_dirs", "a/,b/"], "cascade_thresholds.*cascade_fractions"),                                             # no gate at all
    (["--cascade_dirs", "a/,b/", "--cascade_thresholds", "0.5", "--cascade_towers", "teacher,pupil"], "cascade_towers"),
]


def _inference_main(args, tmp_path):
    from efficientvideoclassification_youtube8m_amd import inference
    return inference.main(COMMON + ["--output_file", str(tmp_path / "p.csv"), "--input_data_pattern", str(tmp_path / "test*.tfrecord")] + args)


def _validate_main(args, tmp_path):
    from efficientvideoclassification_youtube8m_amd import validate
    return validate.main(COMMON + ["--eval_data_pattern", str(tmp_path / "validate*.tfrecord"), "--train_dir", str(tmp_path) + "/"] + args)


@pytest.mark.parametrize("args,match", REFUSED)
def test_inference_refusals(flags, no_device, tmp_path, args, match):
    with pytest.raises(ValueError, match=match):
        _inference_main(args, tmp_path)


@pytest.mark.parametrize("args,match", REFUSED)
def test_validate_refusals(flags, no_device, tmp_path, args, match):
    with pytest.raises(ValueError, match=match):
        _validate_main(args + ["--run_once", "True"], tmp_path)


def test_validate_needs_run_once(flags, no_device, tmp_path):
    with pytest.raises(ValueError, match="cascade_dirs.*run_once"):
        _validate_main(["--cascade_dirs", "a/,b/", "--cascade_thresholds", "0.5"], tmp_path)


# ---- the host bookkeeping ------------------------------------------------------------------------------------------------------------
def test_quota_is_exact_for_dyadic_fractions():
    from efficientvideoclassification_youtube8m_amd import cascade
    for b in (1, 2, 3, 5, 8, 16, 1000, 1024):
        for n_active in sorted({0, 1, b // 2, b}):
            assert cascade.stage_quota(n_active, None, b) == -1
            assert cascade.stage_quota(n_active, 0.0, b) == 0
            assert cascade.stage_quota(n_active, 0.25, b) == min(n_active, (b + 3) // 4)
            assert cascade.stage_quota(n_active, 0.5, b) == min(n_active, (b + 1) // 2)
            assert cascade.stage_quota(n_active, 1.0, b) == n_active
            for f in (None, 0.0, 0.25, 0.5, 1.0):
                assert cascade.stage_quota(n_active, f, b) == ref.quota(n_active, f, b)
    assert cascade.stage_quota(1, 0.25, 1) == 1 and cascade.stage_quota(1, 0.0, 1) == 0       # b = 1: ceil(0.25) = 1
    assert cascade.stage_quota(3, 0.5, 5) == 3 and cascade.stage_quota(2, 0.5, 5) == 2        # the batch's rows, not the active ones


def test_bookkeeping_masks_counts_and_skips_empty_stages():
    from efficientvideoclassification_youtube8m_amd import cascade, ops
    nh = np.array([300, 120, 0, 299, 31, 7], np.int64)
    first = cascade.stage_bookkeeping(0, 3, None, nh, "student", 30, threshold=0.5, fraction=0.5)
    assert first["run"] and first["gate"] and first["rows"] == 6 and first["nh"].tolist() == nh.tolist()
    assert first["threshold"] == 0.5 and first["max_rows"] == 3
    assert first["frames"] == int(ops.host_frame_counts(nh, 30, 5, 2, 300, subsampled=True)[0].sum()) == 10 + 4 + 0 + 9 + 1 + 0
    active = np.array([0, 1, 0, 1, 0, 1], np.uint8)
    mid = cascade.stage_bookkeeping(1, 3, active, nh, "student", 10, fraction=0.25)
    assert mid["run"] and mid["gate"] and mid["rows"] == 3 and mid["nh"].tolist() == [0, 120, 0, 299, 0, 7] and mid["nh"].dtype == np.int64
    assert mid["threshold"] == math.inf and mid["max_rows"] == 2                          # min(3, ceil(0.25 * 6))
    assert mid["frames"] == 12 + 29 + 0
    last = cascade.stage_bookkeeping(2, 3, active.astype(bool), nh, "teacher", 1, threshold=0.9, fraction=1.0)
    assert last["run"] and not last["gate"] and last["frames"] == 120 + 299 + 7
    assert last["frames"] == int(ops.host_frame_counts(last["nh"], 1, 20, 15, 300)[0].sum())
    empty = cascade.stage_bookkeeping(1, 3, np.zeros(6, np.uint8), nh, "teacher", 1, threshold=0.5)
    assert not empty["run"] and not empty["gate"] and empty["rows"] == 0 and empty["frames"] == 0 and not empty["nh"].any()
    one = cascade.stage_bookkeeping(0, 2, None, [150], "teacher", 1, fraction=0.25)       # b = 1
    assert one["run"] and one["gate"] and one["rows"] == 1 and one["max_rows"] == 1 and one["frames"] == 150
    with pytest.raises(ValueError):
        cascade.stage_bookkeeping(1, 2, np.ones(5, np.uint8), nh, "teacher", 1)


def test_frame_accounting_follows_host_frame_counts():
    from efficientvideoclassification_youtube8m_amd import cascade, ops
    rng = np.random.default_rng(4)
    nh = rng.integers(0, 301, 64)
    active = rng.random(64) < 0.5
    for every_n in (10, 30):
        got = cascade.stage_bookkeeping(1, 2, active, nh, "student", every_n)["frames"]
        S = 300 // every_n
        n_used = ops.host_frame_counts(nh, every_n, 5, S // 5, 300, subsampled=True)[0]
        assert got == int(n_used[active].sum())
    assert cascade.stage_bookkeeping(1, 2, active, nh, "teacher", 10)["frames"] == int(nh[active].sum())


def test_gate_checks_of_the_graph():
    from efficientvideoclassification_youtube8m_amd import cascade
    assert cascade.check_gates(3, "top1", None, [0.5, 1]) == ([math.inf, math.inf], [0.5, 1.0])
    assert cascade.check_gates(2, "margin", [0.25], None) == ([0.25], None)
    for args in ((1, "top1", [], None), (9, "top1", [0.5] * 8, None), (2, "entropy", [0.5], None), (2, "top1", None, None),
                 (3, "top1", [0.5], None), (2, "top1", None, [1.25]), (2, "top1", None, [float("nan")])):
        with pytest.raises(ValueError):
            cascade.check_gates(*args)
    with pytest.raises(ValueError):
        cascade.parse_stage(("pupil", 10))


def test_stage_file_format():
    from efficientvideoclassification_youtube8m_amd import cascade
    lines = list(cascade.format_stage_lines([b"vid0", "vid1", "vid2"], np.array([0, 2, 1], np.uint8),
                                            np.array([0.5, 0.123456789, np.nan], np.float32)))
    assert lines == ["vid0,0,0.500000\n", "vid1,2,%f\n" % np.float32(0.123456789), "vid2,1,nan\n"]
    assert cascade.STAGE_FILE_HEADER == "VideoId,Stage,Confidence\n"


# ---- ops ------------------------------------------------------------------------------------------------------------------------
def test_ops_reject_cpu_tensors_and_unknown_kinds():
    import torch
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    pred, merged = torch.rand((4, 64)), torch.zeros((4, 64))
    conf, stage_of = torch.zeros(4), torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(_lib.EvcError, match="CPU"):
        ops.cascade_confidence_rows(pred, "top1", 0, conf, merged, stage_of)
    with pytest.raises(ValueError, match="kind"):
        ops.cascade_confidence_rows(pred, "entropy", 0, conf, merged, stage_of)
    with pytest.raises(_lib.EvcError, match="CPU"):
        ops.cascade_pick_rows(conf, torch.ones(4, dtype=torch.int32), 0.5)
    assert ops.CASCADE_CONFIDENCE == {"top1": 0, "margin": 1} and ops.CASCADE_MAX_ROWS == 16384
