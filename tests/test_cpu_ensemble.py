"""Ensembles without a GPU: the flags and every refusal of inference.check_flags() / validate.check_flags() (before the device is
touched), read_prediction_file, the prior arrays of a batch, the loud CPU-tensor error of ops.ensemble_topk_rows, and the
equivalence DESIGN.md 7.3 states: on tie-free rows the top-k of the dense per-class maximum is the sparse merge (cs/max_ensemble.py)
of the members' own top-k lists."""
import numpy as np
import pytest

import _ensemble_ref as ref

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
    monkeypatch.setattr(inference.ops, "ensemble_topk_rows", touched)
    monkeypatch.setattr(readers, "get_input_evaluation_tensors", touched)
    monkeypatch.setattr(inference, "latest_checkpoint", touched)
    monkeypatch.setattr(validate, "latest_checkpoint", touched)


def _csv(path, lines):
    from efficientvideoclassification_youtube8m_amd import inference
    with open(path, "w") as f:
        f.write(inference.HEADER)
        f.writelines(lines)
    return str(path)


# ---- flags ----------------------------------------------------------------------------------------------------------------------
def test_defaults_mean_no_ensemble(flags):
    from efficientvideoclassification_youtube8m_amd import inference, validate
    for name in ("ensemble_dirs", "ensemble_towers", "ensemble_every_n", "ensemble_weights", "preds_pattern"):
        assert getattr(flags, name) == ""
    assert flags.ensemble_mode == "max"
    assert inference.ensemble_spec() is None
    assert validate.check_flags() is None                                 # and --run_once False is still fine without an ensemble


def test_flag_parsing(flags, tmp_path):
    from efficientvideoclassification_youtube8m_amd import inference
    _csv(tmp_path / "b.csv", [])
    _csv(tmp_path / "a.csv", [])
    flags.parse(["--ensemble_dirs", "dirA/, dirA/,dirB/", "--ensemble_towers", "teacher,student, auto", "--ensemble_every_n", "1, 10,30",
                 "--ensemble_mode", "mean", "--ensemble_weights", "0.5,0.25, 0.125,0.0625,0.0625", "--preds_pattern", str(tmp_path / "*.csv"),
                 "--every_n", "5"])
    spec = inference.ensemble_spec()
    assert spec["dirs"] == ["dirA/", "dirA/", "dirB/"] and spec["towers"] == ["teacher", "student", "auto"]
    assert spec["every_n"] == [1, 10, 30] and spec["mode"] == "mean"
    assert spec["weights"].dtype == np.float32 and spec["weights"].tolist() == [0.5, 0.25, 0.125, 0.0625, 0.0625]
    assert spec["files"] == [str(tmp_path / "a.csv"), str(tmp_path / "b.csv")]        # sorted by name
    flags.reset()
    flags.parse(["--ensemble_dirs", "x/,y/", "--every_n", "20"])
    spec = inference.ensemble_spec()
    assert spec["towers"] == ["auto", "auto"] and spec["every_n"] == [20, 20] and spec["mode"] == "max"
    assert spec["weights"] is None and spec["files"] == []


def _inference_main(args, tmp_path):
    from efficientvideoclassification_youtube8m_amd import inference
    return inference.main(COMMON + ["--output_file", str(tmp_path / "p.csv"), "--input_data_pattern", str(tmp_path / "test*.tfrecord")] + args)


def _nine_files(tmp_path):
    d = tmp_path / "nine"
    d.mkdir()
    for i in range(9):
        _csv(d / ("p%d.csv" % i), [])
    return str(d / "*.csv")


REFUSED = [
    (["--ensemble_dirs", "a/,b/", "--ensemble_towers", "teacher"], "ensemble_towers"),
    (["--ensemble_dirs", "a/,b/", "--ensemble_every_n", "1,2,3"], "ensemble_every_n"),
    (["--ensemble_towers", "teacher"], "ensemble_towers"),                                         # a list for no members
    (["--ensemble_dirs", "a/,b/", "--ensemble_towers", "teacher,pupil"], "ensemble_towers"),
    (["--ensemble_dirs", "a/,b/", "--ensemble_mode", "median"], "ensemble_mode"),
    (["--ensemble_dirs", "a/,b/", "--ensemble_mode", "max", "--ensemble_weights", "0.5,0.5"], "ensemble_weights"),
    (["--ensemble_dirs", "a/,b/", "--ensemble_mode", "mean", "--ensemble_weights", "0.5,0.25,0.25"], "ensemble_weights"),
    (["--ensemble_dirs", ",".join("d%d/" % i for i in range(9))], "ensemble_dirs"),
]


@pytest.mark.parametrize("args,match", REFUSED)
def test_inference_refusals(flags, no_device, tmp_path, args, match):
    with pytest.raises(ValueError, match=match):
        _inference_main(args, tmp_path)


def test_inference_refuses_bad_prediction_file_sets(flags, no_device, tmp_path):
    with pytest.raises(ValueError, match="matches no file"):
        _inference_main(["--ensemble_dirs", "a/", "--preds_pattern", str(tmp_path / "none*.csv")], tmp_path)
    flags.reset()
    with pytest.raises(ValueError, match="at most 8"):
        _inference_main(["--ensemble_dirs", "a/", "--preds_pattern", _nine_files(tmp_path)], tmp_path)
    flags.reset()
    one = _csv(tmp_path / "one.csv", [])
    with pytest.raises(ValueError, match="preds_pattern without --ensemble_dirs"):
        _inference_main(["--preds_pattern", one], tmp_path)
    flags.reset()
    with pytest.raises(ValueError, match="ensemble_weights"):              # the files count: 1 member + 1 file needs 2 weights
        _inference_main(["--ensemble_dirs", "a/", "--preds_pattern", one, "--ensemble_mode", "mean", "--ensemble_weights", "1.0"], tmp_path)


def _validate_main(args, tmp_path):
    from efficientvideoclassification_youtube8m_amd import validate
    return validate.main(COMMON + ["--eval_data_pattern", str(tmp_path / "validate*.tfrecord"), "--train_dir", str(tmp_path) + "/"] + args)


@pytest.mark.parametrize("args,match", REFUSED)
def test_validate_refusals(flags, no_device, tmp_path, args, match):
    with pytest.raises(ValueError, match=match):
        _validate_main(args + ["--run_once", "True"], tmp_path)


def test_validate_needs_run_once_and_takes_no_prediction_files(flags, no_device, tmp_path):
    with pytest.raises(ValueError, match="run_once"):
        _validate_main(["--ensemble_dirs", "a/,b/"], tmp_path)
    flags.reset()
    with pytest.raises(ValueError, match="run_once"):
        _validate_main(["--ensemble_dirs", "a/,b/", "--run_once", "False"], tmp_path)
    flags.reset()
    with pytest.raises(ValueError, match="preds_pattern"):
        _validate_main(["--ensemble_dirs", "a/,b/", "--run_once", "True", "--preds_pattern", _csv(tmp_path / "one.csv", [])], tmp_path)


# ---- prediction files -----------------------------------------------------------------------------------------------------------
def test_read_prediction_file_round_trip(tmp_path):
    from efficientvideoclassification_youtube8m_amd import inference
    rng = np.random.default_rng(0)
    ids = ["vid%02d" % i for i in range(6)]
    vals = np.sort(rng.random((6, 20), dtype=np.float32), axis=1)[:, ::-1].copy()
    idx = np.stack([rng.choice(4716, 20, replace=False) for _ in ids]).astype(np.int32)
    lines = list(inference.format_lines(ids, vals, idx))
    path = _csv(tmp_path / "p.csv", lines + ["empty,\n"])
    table = inference.read_prediction_file(path)
    assert list(table) == ids + ["empty"] and table["empty"][0].size == 0
    for r, vid in enumerate(ids):
        cls, conf = table[vid]
        assert cls.dtype == np.int32 and conf.dtype == np.float32
        assert cls.tolist() == idx[r].tolist()
        assert np.abs(conf.astype(np.float64) - vals[r]).max() <= 0.5e-6 + 2.0 ** -24    # "%f" rounding + the float32 of the text
    # what was parsed prints as the same text
    again = list(inference.format_lines(ids, np.stack([table[v][1] for v in ids]), np.stack([table[v][0] for v in ids])))
    assert again == lines


def test_read_prediction_file_rejects(tmp_path):
    from efficientvideoclassification_youtube8m_amd import inference
    with pytest.raises(ValueError, match="twice"):
        inference.read_prediction_file(_csv(tmp_path / "a.csv", ["v0,3 0.5 7 0.4 3 0.1\n"]))
    with pytest.raises(ValueError, match="outside"):
        inference.read_prediction_file(_csv(tmp_path / "b.csv", ["v0,3 0.5 4716 0.4\n"]))
    with pytest.raises(ValueError, match="outside"):
        inference.read_prediction_file(_csv(tmp_path / "c.csv", ["v0,-1 0.5\n"]))
    inference.read_prediction_file(_csv(tmp_path / "d.csv", ["v0,3 0.5 12 0.4\n"]), num_classes=13)
    with pytest.raises(ValueError, match="outside"):
        inference.read_prediction_file(_csv(tmp_path / "d.csv", ["v0,3 0.5 12 0.4\n"]), num_classes=12)
    pairs = lambda n: " ".join("%d 0.5" % c for c in range(n))
    assert inference.read_prediction_file(_csv(tmp_path / "e.csv", ["v0," + pairs(256) + "\n"]))["v0"][0].size == 256
    with pytest.raises(ValueError, match="at most 256"):
        inference.read_prediction_file(_csv(tmp_path / "f.csv", ["v0," + pairs(257) + "\n"]))
    with pytest.raises(ValueError, match="first line"):
        p = tmp_path / "g.csv"
        p.write_text("v0,3 0.5\n")
        inference.read_prediction_file(str(p))
    with pytest.raises(ValueError, match="class conf"):
        inference.read_prediction_file(_csv(tmp_path / "h.csv", ["v0,3 0.5 7\n"]))


def test_prior_arrays_of_a_batch(tmp_path):
    from efficientvideoclassification_youtube8m_amd import inference
    fa = _csv(tmp_path / "a.csv", ["v0,3 0.5 7 0.25\n", "v1,9 0.125\n", "v2,\n"])
    fb = _csv(tmp_path / "b.csv", ["v2,1 0.75 2 0.5 3 0.25\n", "v1,7 1.0\n", "v0,3 0.0625\n"])
    tables = [inference.read_prediction_file(f) for f in (fa, fb)]
    kp = inference.prior_list_length(tables)
    assert kp == 3
    idx, val = inference.gather_priors(tables, [fa, fb], [b"v2", "v0", "v1"], kp)      # the batch's order, ids as bytes or str
    assert idx.dtype == np.int32 and val.dtype == np.float32 and idx.shape == val.shape == (2, 3, 3)
    assert idx.tolist() == [[[-1, -1, -1], [3, 7, -1], [9, -1, -1]], [[1, 2, 3], [3, -1, -1], [7, -1, -1]]]
    assert val.tolist() == [[[0, 0, 0], [0.5, 0.25, 0], [0.125, 0, 0]], [[0.75, 0.5, 0.25], [0.0625, 0, 0], [1.0, 0, 0]]]
    out = (np.full((2, 1, 3), 99, np.int32), np.full((2, 1, 3), 99, np.float32))      # arrays given by the caller are overwritten whole
    got = inference.gather_priors(tables, [fa, fb], ["v1"], kp, out=out)
    assert got[0] is out[0] and out[0].tolist() == [[[9, -1, -1]], [[7, -1, -1]]] and out[1].tolist() == [[[0.125, 0, 0]], [[1.0, 0, 0]]]
    with pytest.raises(KeyError) as e:
        inference.gather_priors(tables, [fa, fb], ["v0", "v9"], kp)
    assert "v9" in str(e.value) and fa in str(e.value)
    assert inference.prior_list_length([{}]) == 1                                      # kp >= 1 for files of empty lists


# ---- ops ------------------------------------------------------------------------------------------------------------------------
def test_ops_rejects_cpu_tensors():
    import torch
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    x = torch.rand((4, 64))
    with pytest.raises(_lib.EvcError, match="CPU"):
        ops.ensemble_topk_rows([x, x], 5)
    with pytest.raises(_lib.EvcError, match="CPU"):
        ops.ensemble_topk_rows([x], 0, mode="mean", dense=True)


# ---- the equivalence of DESIGN.md 7.3 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,rows,cols,k", [(1, 5, 64, 20), (2, 16, 4716, 20), (3, 8, 4716, 20), (8, 4, 4716, 20), (4, 8, 300, 1), (3, 6, 257, 256)])
def test_dense_max_equals_sparse_merge_on_tie_free_rows(M, rows, cols, k):
    """A class in the top-k of the per-class maximum is in the top-k of the member that attains it, so merging the members' own
    top-k lists (cs/max_ensemble.py) loses nothing.  The rows are drawn tie-free: all M * cols values of a row are distinct."""
    rng = np.random.default_rng(M * 1000 + cols)
    n = M * cols
    grid = (np.arange(1, n + 1, dtype=np.float64) / (n + 1)).astype(np.float32)
    assert np.unique(grid).size == n
    members = [np.empty((rows, cols), np.float32) for _ in range(M)]
    for r in range(rows):
        perm = rng.permutation(grid).reshape(M, cols)
        for m in range(M):
            members[m][r] = perm[m]
    dense_val, dense_idx = ref.topk(ref.combine_max(members), k)
    own = [ref.topk(x, k) for x in members]
    for r in range(rows):
        cls, conf = ref.sparse_merge([(own[m][1][r], own[m][0][r]) for m in range(M)], k)
        assert cls.tolist() == dense_idx[r].tolist()
        assert np.array_equal(conf.view(np.uint32), dense_val[r].view(np.uint32))
