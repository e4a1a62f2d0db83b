"""Content-aware student frames on the GPU (--student_sampling change | segment_change): the key kernel and the scored table against their
numpy restatement (tests/_frame_change_ref.py), the gathering pass and the graphs against the uniform ones on host-rearranged frames, the
keys computed once per batch by the graphs that own several students, and the binaries.

Everything is compared with ==.  The uint8 keys are exact integers.  The f32 key tests use integer-valued frames in [-8, 8]: every partial
sum is an integer below 2^24, so every summation order gives the same bits; on general f32 frames only repeatability is asserted (the
contract leaves near-ties to the device's summation order), and the tables expected of the graphs on such frames are the reference's
ranking of the keys the device computed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _frame_change_ref as ref
import _frame_select_ref as sel_ref
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIRST = 0xFFFFFFFF
# the issue's two shapes (the second: unaligned rows, the narrow accesses), and small ones of every other path of the key kernel:
# bytes by single bytes (F = 101), rows of 2 .. 5 KB kept in registers (F = 2064 bytes), rows too long for that (16-byte pieces from memory:
# 5136 bytes / 1284 floats), floats one by one (F = 101)
SHAPES = [(6, 300, 1152), (3, 37, 100)]
EXTRA_U8 = [(2, 20, 101), (2, 20, 2064), (2, 20, 5136)]
EXTRA_F32 = [(2, 20, 101), (2, 20, 1284)]


@pytest.fixture(scope="module")
def ops():
    from efficientvideoclassification_youtube8m_amd import ops as o
    return o


def _counts(B, T):
    """0, 1, 2, T - 1, T and a value above T at B = 6; the three longest at B = 3, the two longest at B = 2."""
    return np.array([T + 7, T, T - 1, 2, 1, 0][:B] if B != 2 else [T, T - 7], np.int32)


def _byte_videos(B, T, F, seed):
    """Row 0 random bytes; row 1 alternates two frames A, B, A, B ... (all keys equal); row 2 alternates all-0 and all-255 (F * 65025);
    row 3 constant (all keys 0); the others random."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (B, T, F), dtype=np.uint8)
    if B > 2:
        q[1, 0::2], q[1, 1::2] = q[1, 0], q[1, 1]
        q[2, 0::2], q[2, 1::2] = 0, 255
    if B > 3:
        q[3] = q[3, 0]
    return q


def _dev_keys(ops, x, n):
    return ops.frame_change_keys(torch.from_numpy(x).to(DEV), torch.from_numpy(n).to(DEV)).cpu().numpy().view(np.uint32)


# ---- 1. keys ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,F", SHAPES + EXTRA_U8)
def test_keys_bytes_are_exact(ops, B, T, F):
    q, n = _byte_videos(B, T, F, seed=F), _counts(B, T)
    want = ref.keys(q, n)
    got = _dev_keys(ops, q, n)
    assert got.shape == (B, T) and np.array_equal(got, want), np.argwhere(got != want)[:4]
    if B > 2:
        live = min(int(n[2]), T)
        assert live < 2 or (want[2, 1:live] == F * 65025).all()                             # the accumulator's full width
        assert (want[1, 1:min(int(n[1]), T)] == want[1, 1]).all()
    if (B, T, F) == SHAPES[0]:                                                            # the counts turned round: the constant row is live
        n2 = n[::-1].copy()
        want2 = ref.keys(q, n2)
        assert (want2[3, 1:] == 0).all() and want2[3, 0] == FIRST
        assert np.array_equal(_dev_keys(ops, q, n2), want2)


@pytest.mark.parametrize("B,T,F", SHAPES)
@pytest.mark.parametrize("offset", [4, 1])
def test_keys_bytes_on_an_offset_view(ops, B, T, F, offset):
    """The first row starts `offset` bytes into a buffer: 4-byte accesses (offset 4) or single bytes (offset 1), never 16-byte ones."""
    q, n = _byte_videos(B, T, F, seed=5), _counts(B, T)
    buf = torch.zeros(offset + B * T * F, dtype=torch.uint8, device=DEV)
    view = buf[offset:].view(B, T, F)
    view.copy_(torch.from_numpy(q))
    assert view.is_contiguous() and view.data_ptr() % 16 == offset
    got = ops.frame_change_keys(view, torch.from_numpy(n).to(DEV)).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, ref.keys(q, n))


@pytest.mark.parametrize("B,T,F", SHAPES + EXTRA_F32)
def test_keys_floats_are_exact_on_integer_frames(ops, B, T, F):
    rng = np.random.default_rng(F + 1)
    x = rng.integers(-8, 9, (B, T, F)).astype(np.float32)                                # (d^2 <= 256, F d^2 < 2^24: every order is exact)
    n = _counts(B, T)
    if B > 2:
        x[1, 0::2], x[1, 1::2] = x[1, 0], x[1, 1]
    want = ref.keys(x, n)
    got = _dev_keys(ops, x, n)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    x[0, 5, F // 2] = np.nan                                                              # one NaN: that frame's key and its successor's
    want = ref.keys(x, n)
    assert want[0, 5] == FIRST and want[0, 6] == FIRST and want[0, 4] != FIRST and want[0, 7] != FIRST
    got = _dev_keys(ops, x, n)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


@pytest.mark.parametrize("B,T,F", SHAPES + EXTRA_F32)
def test_keys_floats_repeat(ops, B, T, F):
    x = np.random.default_rng(F).standard_normal((B, T, F)).astype(np.float32)
    n = _counts(B, T)
    a, b = _dev_keys(ops, x, n), _dev_keys(ops, x, n)
    assert np.array_equal(a, b)
    want = ref.keys(x, n)                                                                  # no order asserted; the value itself to f32 rounding
    live = np.arange(T)[None, :] < np.minimum(n, T)[:, None]
    live[:, 0] = False
    assert np.array_equal(a[~live], want[~live])
    assert np.allclose(a[live].view(np.float32), want[live].view(np.float32), rtol=F * 2.0 ** -23, atol=0)


# ---- 2. tables ----------------------------------------------------------------------------------------------------------------------
def _frame_numbers(T, every_n):
    return np.array([0, 1, 2, every_n - 1, every_n, 55, 79, T - 1, T, T + 7, T // 2, 17], np.int32)          # B = 12


def _planted_keys(B, T, seed):
    """Few distinct values (ties everywhere), a row of equal keys, a falling and a rising row, a row of real byte keys."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 5, (B, T)).astype(np.uint32)
    k[1] = 7
    k[2] = np.arange(T, 0, -1)
    k[3] = np.arange(T)
    k[4] = rng.integers(0, 2 ** 32, T, dtype=np.uint64).astype(np.uint32)                # the full width, above 2^31 too
    k[5:, 0] = FIRST
    k[6, T // 3:T // 3 + 9] = 0xFFFFFFF0                                                  # the big jumps sit together
    return k


@pytest.mark.parametrize("T,every_n", [(300, 1), (300, 2), (300, 10), (300, 30), (60, 2), (1024, 4)])
def test_tables_are_exact(ops, T, every_n):
    n = _frame_numbers(T, every_n)
    nd = torch.from_numpy(n).to(DEV)
    S = T // every_n
    k_dev = ops.frame_counts(torch.from_numpy(np.minimum(n, T)).to(DEV), every_n, 1, S, T, subsampled=True)[0].cpu().numpy()
    q = _byte_videos(12, T, 64, seed=T + every_n)
    real = ref.keys(q, n)
    assert np.array_equal(_dev_keys(ops, q, n), real)
    for keys in (real, _planted_keys(12, T, every_n)):
        kd = torch.from_numpy(keys.view(np.int32)).to(DEV)
        for strategy in ref.STRATEGIES:
            got = ops.student_frame_select_scored(nd, kd, T, every_n, strategy).cpu().numpy()
            want = ref.table(keys, n, T, every_n, strategy)
            assert got.dtype == np.int32 and got.shape == (12, S)
            assert np.array_equal(got, want), (strategy, np.argwhere(got != want)[:4])
            assert np.array_equal((got >= 0).sum(1), k_dev), strategy


# ---- 3. limits ----------------------------------------------------------------------------------------------------------------------
def test_limits(ops):
    from efficientvideoclassification_youtube8m_amd import _lib
    nd = torch.tensor([300, 200], dtype=torch.int32, device=DEV)
    xf = torch.zeros((2, 4, 8), dtype=torch.float32, device=DEV)
    xq = torch.zeros((2, 4, 8), dtype=torch.uint8, device=DEV)
    keys = torch.full((2, 1100), 12345, dtype=torch.int32, device=DEV)
    src = torch.full((2, 1100), 12345, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()                                                            # noqa: E731
    bad_shape, bad_arg = r"\(-1\)", r"\(-5\)"
    for args, code in (((p(xf), None, p(nd), 2, 1025, 8), bad_shape), ((None, None, p(nd), 2, 4, 8), bad_arg),
                       ((p(xf), p(xq), p(nd), 2, 4, 8), bad_arg), ((None, p(xq), p(nd), 2, 4, 66052), bad_shape),
                       ((p(xf), None, p(nd), 0, 4, 8), bad_shape), ((p(xf), None, p(nd), 2, 4, 0), bad_shape),
                       ((p(xf), None, None, 2, 4, 8), bad_arg)):
        with pytest.raises(_lib.EvcError, match=code):
            _lib.call("evc_frame_change_keys", *args, p(keys), None)
    for kw, code in ((dict(strategy=5), bad_arg), (dict(strategy=8), bad_arg), (dict(strategy=0), bad_arg), (dict(T=1025), bad_shape),
                     (dict(every_n=0), bad_shape), (dict(every_n=301), bad_shape), (dict(B=0), bad_shape)):
        a = dict(B=2, T=300, every_n=10, strategy=6)
        a.update(kw)
        with pytest.raises(_lib.EvcError, match=code):
            _lib.call("evc_student_frame_select_scored", p(nd), p(keys), a["B"], a["T"], a["every_n"], a["strategy"], p(src), None)
    torch.cuda.synchronize()
    assert (keys == 12345).all() and (src == 12345).all()                                # nothing was launched
    with pytest.raises(ValueError, match="frames are needed"):
        ops.student_frame_select(nd, 300, 10, "change")


# ---- 4. the gathering pass ----------------------------------------------------------------------------------------------------------
B2, T2, EVERY_N, C2 = 3, 300, 10, 5
MODES = [dict(), dict(split=True), dict(split="f16", f16_segments=1), dict(split="f16", f16_segments=2), dict(split="f16", f16_segments=3),
         dict(split="wide"), dict(split="f16", f16_segments=1, fp8_tail=True)]           # every form input_image_args / input_split ask for


@pytest.fixture(scope="module")
def frames():
    out = {}
    for F in (128, 1152):
        q, x, n, _ = mm.synthetic_batch(B2, seed=11 + F, feature_size=F, vocab_size=8, dtype=np.float32)
        n[:] = (300, 137, 41)
        out[F] = (q, mm.dequantize(q.astype(np.float32)).astype(np.float32), n)         # (x NOT zeroed beyond n: f32 input has no pad rule)
    return out


def _plans(ops, nd, n):
    S = T2 // EVERY_N
    _, l1, _ = ops.frame_counts(nd, EVERY_N, C2, S // C2, T2, subsampled=True)
    _, l1h, _ = ops.host_frame_counts(n, EVERY_N, C2, S // C2, T2, subsampled=True)
    return [None, ops.RowPlan(l1, l1h, S // C2)]


def _same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def _live(view, plan):
    views = view if isinstance(view, tuple) else (view,)
    if plan is None:
        return views
    keep = (plan.lens > 0).nonzero().flatten()
    return tuple(v[:, keep] for v in views)


@pytest.mark.parametrize("F", [128, 1152])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("strategy", ref.STRATEGIES)
def test_gather_equals_existing_entry_on_rearranged_frames(ops, frames, F, u8, strategy):
    q, x, n = frames[F]
    nd = torch.from_numpy(n).to(DEV)
    host = q if u8 else x
    inp = torch.from_numpy(host).to(DEV)
    keys = ops.frame_change_keys(inp, nd)
    keys_h = keys.cpu().numpy().view(np.uint32)
    if u8:
        assert np.array_equal(keys_h, ref.keys(q, n))
    src = ops.student_frame_select_scored(nd, keys, T2, EVERY_N, strategy)
    src_h = src.cpu().numpy()
    assert np.array_equal(src_h, ref.table(keys_h, n, T2, EVERY_N, strategy))
    inp_p = torch.from_numpy(sel_ref.rearrange(host, src_h, EVERY_N)).to(DEV)
    # uint8 zeros are not zero frames: x' gets its zero rows from the pad rule, which then starts exactly behind the last selected slot
    k = (src_h >= 0).sum(1)
    nd_p = torch.from_numpy((k * EVERY_N).astype(np.int32)).to(DEV)
    for plan in _plans(ops, nd, n):
        for mode in MODES:
            want = ops.l2norm_chunk(inp_p, 20, EVERY_N, C2, teacher_view=False, num_frames=nd_p if u8 else None, plan2=plan, **mode)[1]
            got = ops.l2norm_chunk_sel(inp, src, EVERY_N, C2, num_frames=nd if u8 else None, plan2=plan, **mode)
            assert _same(_live(got, plan), _live(want, plan)), (mode, plan is not None)
        if u8:
            want = ops.l2norm_chunk_int(inp_p, nd_p, 20, EVERY_N, C2, plan2=plan, teacher_view=False)[1]
            got = ops.l2norm_chunk_int_sel(inp, nd, src, EVERY_N, C2, plan2=plan)
            assert _same(_live(got, plan), _live(want, plan)), plan is not None


# ---- 5. the graphs ------------------------------------------------------------------------------------------------------------------
GRAPH_KW = dict(every_n=10, feature_size=128, vocab_size=50, lstm_cells=64, device=DEV)


@pytest.fixture(scope="module")
def batch():
    q, x, n, labels = mm.synthetic_batch(6, seed=3, feature_size=128, vocab_size=50, dtype=np.float32)
    n[0], n[1] = 300, 79
    return q, x, n, labels


@pytest.mark.parametrize("precision,u8", [("bf16", False), ("high", True)])
@pytest.mark.parametrize("strategy", ref.STRATEGIES)
def test_eval_graph_equals_uniform_graph_on_rearranged_frames(ops, batch, precision, u8, strategy):
    from efficientvideoclassification_youtube8m_amd.distill import EvalGraph
    q, x, n, labels = batch
    host = q if u8 else x
    g = EvalGraph(6, precision=precision, student_sampling=strategy, **GRAPH_KW)          # teacher + student
    u = EvalGraph(6, precision=precision, **GRAPH_KW)
    u.restore({**g.teacher.state_dict(), **g.student.state_dict()})
    hd, nd, yd = torch.from_numpy(host).to(DEV), torch.from_numpy(n).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV)
    out = g.step(hd, yd, nd, num_frames_host=n)
    pred, state, t_pred, t_state = (out[k].clone() for k in ("predictions", "student_state", "teacher_predictions", "teacher_state"))
    keys = ops.frame_change_keys(hd, nd).cpu().numpy().view(np.uint32)
    if u8:
        assert np.array_equal(keys, ref.keys(q, n))
    src = g.last_frame_table.cpu().numpy()
    assert np.array_equal(src, ref.table(keys, n, 300, 10, strategy))
    plain = u.step(hd, yd, nd, num_frames_host=n)
    assert torch.equal(t_pred, plain["teacher_predictions"]) and torch.equal(t_state, plain["teacher_state"])      # the teacher: untouched
    assert not torch.equal(pred, plain["predictions"])                                   # and it is not the uniform student of x
    out_u = u.step(torch.from_numpy(sel_ref.rearrange(host, src, 10)).to(DEV), yd, nd, num_frames_host=n)
    assert torch.equal(pred, out_u["predictions"]) and torch.equal(state, out_u["student_state"])
    assert torch.equal(out["num_frames"], out_u["num_frames"])


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = tmp_path_factory.mktemp("frame_change") / "res.pt"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_frame_change_child.py"), str(out)],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = torch.load(str(out))
    print(res)
    assert res["deterministic"] == "1" and res["same_start"] and res["keys_repeat"]
    return res


@pytest.mark.parametrize("strategy", ref.STRATEGIES)
def test_student_only_step_equals_uniform_step_on_rearranged_frames(child, strategy):
    assert child[strategy + "_table"] and child[strategy + "_moved"] and child[strategy + "_is_not_uniform"]
    assert child[strategy + "_loss_equal"], child[strategy + "_loss"]
    assert child[strategy + "_pred_equal"] and child[strategy + "_weights_equal"]
    assert child[strategy + "_key_launches"] == 1


def test_teacher_is_untouched_by_the_students_frames(child):
    assert child["teacher_student_table"] and child["student_differs"]
    assert child["teacher_loss_equal"], child["teacher_loss"]
    assert child["teacher_pred_equal"] and child["teacher_weights_equal"]


# ---- 6. the keys once per batch -------------------------------------------------------------------------------------------------------
def test_serial_students_share_the_keys(child):
    assert child["serial_key_launches"] == [1, 1] and child["serial_unscored_key_launches"] == 0
    assert child["serial_tables"]


def test_ensemble_members_share_the_keys(ops, batch, monkeypatch):
    from efficientvideoclassification_youtube8m_amd.distill import EnsembleGraph, EvalGraph
    q, x, n, labels = batch
    kw = {k: v for k, v in GRAPH_KW.items() if k != "every_n"}
    members = [("student", 10, "change"), ("student", 30, "segment_change"), ("teacher", 1, "change"), ("student", 10, "first")]
    g = EnsembleGraph(6, members, **kw)
    qd, nd, yd = torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV)
    calls, inner = [], ops.frame_change_keys

    def counted(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    monkeypatch.setattr(ops, "frame_change_keys", counted)
    for _ in range(2):
        del calls[:]
        preds = [p.clone() for p in g.step(qd, yd, nd, num_frames_host=n)]
        assert len(calls) == 1 and len(preds) == 4
    keys = ref.keys(q, n)
    for m, (_, every_n, word) in zip(g.members[:2], members[:2]):
        assert np.array_equal(m.last_frame_table.cpu().numpy(), ref.table(keys, n, 300, every_n, word))
    # each member computes what a graph of its own computes (which then takes the keys itself)
    for m, (_, every_n, word), p in zip(g.members[:2], members[:2], preds[:2]):
        own = EvalGraph(6, every_n=every_n, student_only=True, student_sampling=word, **kw)
        own.restore(m.student.state_dict())
        del calls[:]
        assert torch.equal(own.step(qd, yd, nd, num_frames_host=n)["predictions"], p) and len(calls) == 1
    del calls[:]
    EnsembleGraph(6, [("student", 10, "first"), ("teacher", 1)], **kw).step(qd, yd, nd, num_frames_host=n)
    assert not calls


# ---- 7. the binaries ------------------------------------------------------------------------------------------------------------------
COMMON = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model",
          "HierarchicalLstmModel", "--gpu", "0", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64",
          "--every_n", "10", "--num_readers", "2"]


def test_binaries_with_change(tmp_path, caplog):
    import logging
    from efficientvideoclassification_youtube8m_amd import inference, readers, train, train_convert_model, validate
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    data = tmp_path / "yt8m"
    readers.write_synthetic_frame_dataset(str(data), 2, 7, feature_sizes=(64, 64), min_frames=60, max_frames=310, seed=2, prefix="test")
    pattern = str(data / "test*.tfrecord")
    tdir = str(tmp_path / "model_train") + "/"
    word = ["--student_sampling", "change"]
    try:
        FLAGS.reset()
        train.main(COMMON + word + ["--synthetic_videos", "16", "--batch_size", "8", "--num_epochs", "1", "--train_data_pattern", "synthetic",
                                    "--train_dir", tdir, "--start_new_model", "True"])
        sd = torch.load(train.latest_checkpoint(tdir))
        assert sd["student_sampling"] == "change" and sd["global_step"] == 4
        ev = ["--eval_data_pattern", "synthetic", "--synthetic_videos", "16", "--train_dir", tdir, "--batch_size", "8", "--run_once", "True"]
        with caplog.at_level(logging.WARNING):
            FLAGS.reset()
            info = validate.main(COMMON + word + ev)
            assert not [r for r in caplog.records if "trained with" in r.getMessage()]
            FLAGS.reset()
            info2 = validate.main(COMMON + ["--student_sampling", "segment_change"] + ev)      # another word: a warning, and the flag is used
            assert [r for r in caplog.records if "trained with change" in r.getMessage()]
        for key in ("avg_hit_at_one", "avg_perr", "avg_loss", "gap"):
            assert np.isfinite(info[key]) and np.isfinite(info2[key]), key
        assert info["avg_loss"] != info2["avg_loss"]
        FLAGS.reset()
        ck = train_convert_model.main(["--train_dir", tdir] + word)
        assert torch.load(ck)["student_sampling"] == "change"
        fdir = train_convert_model.finetune_dir(tdir)

        def run(name, extra):
            out = str(tmp_path / name)
            FLAGS.reset()
            st = inference.main(COMMON + ["--input_data_pattern", pattern, "--output_file", out, "--batch_size", "5", "--top_k", "20",
                                          "--train_dir", fdir] + extra)
            assert st["videos"] == 14 and len(inference.read_prediction_file(out)) == 14
            return open(out, "rb").read()
        texts = {w: run(w + ".csv", ["--student_sampling", w]) for w in ("change", "segment_change", "uniform")}
        assert texts["change"] == run("change2.csv", word)                                # byte-identical: nothing is drawn
        assert len(set(texts.values())) == 3
        ens = run("ens.csv", ["--ensemble_dirs", fdir + "," + fdir, "--ensemble_sampling", "change,segment_change", "--ensemble_mode", "max"])
        assert ens not in texts.values()
    finally:
        FLAGS.reset()
