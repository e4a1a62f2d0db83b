"""Student frame selection on the GPU (--student_sampling): the table kernel against its numpy restatement (exact), the gathering input pass
against the existing entries (bitwise), the graphs against the uniform graphs on a host-rearranged input (bitwise), and the binaries.

Everything is compared with ==: the table is integer arithmetic, the gathering pass runs the row code of evc_l2norm_chunk_fwd on the
same frame values, and a graph that is handed the same student image computes the same numbers (the training steps in a child process
under EVC_DETERMINISTIC=1, where no floating-point atomics are left on the path)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _frame_select_ref as ref
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from efficientvideoclassification_youtube8m_amd import ops as o
    return o


# ---- 1. the table -------------------------------------------------------------------------------------------------------------------
def _frame_numbers(T, every_n):
    return np.array([0, 1, 2, every_n - 1, every_n, 55, 79, 299, 300, T + 7, 150, 17], np.int32)          # B = 12


@pytest.mark.parametrize("T,every_n", [(300, 1), (300, 2), (300, 10), (300, 30), (60, 2)])
@pytest.mark.parametrize("row0", [0, 36])
def test_table_is_exact(ops, T, every_n, row0):
    n = _frame_numbers(T, every_n)
    nd = torch.from_numpy(n).to(DEV)
    S = T // every_n
    # the existing count of the frames the video has inside the tensor, n = min(num_frames, T), as the table defines k
    k_dev = ops.frame_counts(torch.from_numpy(np.minimum(n, T)).to(DEV), every_n, 5, S // 5, T, subsampled=True)[0].cpu().numpy()
    for strategy in ref.STRATEGIES:
        for seed, draw in ((0, 0), (0xDEADBEEF, 77)):
            got = ops.student_frame_select(nd, T, every_n, strategy, seed=seed, draw=draw, row0=row0).cpu().numpy()
            want = ref.table(n, T, every_n, strategy, seed=seed, draw=draw, row0=row0)
            assert got.dtype == np.int32 and got.shape == (12, S)
            assert np.array_equal(got, want), (strategy, seed, np.argwhere(got != want)[:4])
            if strategy != "uniform":
                assert np.array_equal((got >= 0).sum(1), k_dev), strategy
    a = ops.student_frame_select(nd, T, every_n, "random", seed=1, draw=0, row0=row0).cpu().numpy()
    if (n.clip(0, T) * S // T).max() < np.minimum(n, T).max():               # (every_n = 1 takes nearly every frame: little to draw)
        assert (a != ops.student_frame_select(nd, T, every_n, "random", seed=2, draw=0, row0=row0).cpu().numpy()).any()
        assert (a != ops.student_frame_select(nd, T, every_n, "random", seed=1, draw=1, row0=row0).cpu().numpy()).any()


def test_table_limits(ops):
    from efficientvideoclassification_youtube8m_amd import _lib
    nd = torch.tensor([1000, 1024], dtype=torch.int32, device=DEV)
    got = ops.student_frame_select(nd, 1024, 4, "random", seed=3).cpu().numpy()                   # the largest T: four passes of 256
    assert np.array_equal(got, ref.table([1000, 1024], 1024, 4, "random", seed=3))
    for kw in (dict(T=1025), dict(T=0), dict(every_n=0), dict(every_n=301), dict(strategy=6), dict(strategy=-1), dict(row0=-1), dict(B=0)):
        a = dict(B=2, T=300, every_n=10, strategy=1, row0=0)
        a.update(kw)
        src = torch.empty((2, 1024), dtype=torch.int32, device=DEV)
        with pytest.raises(_lib.EvcError, match=r"\((-1|-5)\)"):
            _lib.call("evc_student_frame_select", nd.data_ptr(), a["B"], a["T"], a["every_n"], a["strategy"], 0, 0, a["row0"], src.data_ptr(), None)
    with pytest.raises(ValueError, match="evenly"):
        ops.student_frame_select(nd, 300, 10, "evenly")


# ---- 2. the gathering pass ---------------------------------------------------------------------------------------------------------
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


def _live(view, plan, ops):
    """The rows of an image (or tuple of images) that the kernels write: with a plan, slots of length-0 rows are left as allocated."""
    views = view if isinstance(view, tuple) else (view,)
    if plan is None:
        return views
    keep = (plan.lens > 0).nonzero().flatten()
    return tuple(v[:, keep] for v in views)


@pytest.mark.parametrize("F", [128, 1152])
@pytest.mark.parametrize("u8", [False, True])
def test_gather_uniform_table_is_the_existing_view(ops, frames, F, u8):
    q, x, n = frames[F]
    nd = torch.from_numpy(n).to(DEV)
    inp = torch.from_numpy(q if u8 else x).to(DEV)
    src = ops.student_frame_select(nd, T2, EVERY_N, "uniform")
    for plan in _plans(ops, nd, n):
        for mode in MODES:
            kw = dict(num_frames=nd if u8 else None, plan2=plan, **mode)
            want = ops.l2norm_chunk(inp, 20, EVERY_N, C2, teacher_view=False, **kw)[1]
            got = ops.l2norm_chunk_sel(inp, src, EVERY_N, C2, **kw)
            assert _same(_live(got, plan, ops), _live(want, plan, ops)), (mode, plan is not None)
        if u8:
            want = ops.l2norm_chunk_int(inp, nd, 20, EVERY_N, C2, plan2=plan, teacher_view=False)[1]
            got = ops.l2norm_chunk_int_sel(inp, nd, src, EVERY_N, C2, plan2=plan)
            assert len(got) == 3 and _same(_live(got, plan, ops), _live(want, plan, ops)), plan is not None


@pytest.mark.parametrize("F", [128, 1152])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("strategy", ["random", "first_middle_last"])
def test_gather_equals_existing_entry_on_rearranged_frames(ops, frames, F, u8, strategy):
    q, x, n = frames[F]
    nd = torch.from_numpy(n).to(DEV)
    src = ops.student_frame_select(nd, T2, EVERY_N, strategy, seed=9, draw=2, row0=5)
    src_h = src.cpu().numpy()
    assert np.array_equal(src_h, ref.table(n, T2, EVERY_N, strategy, seed=9, draw=2, row0=5))
    host = q if u8 else x
    inp, inp_p = torch.from_numpy(host).to(DEV), torch.from_numpy(ref.rearrange(host, src_h, EVERY_N)).to(DEV)
    # uint8 zeros are not zero frames: x' gets its zero rows from the pad rule, which then starts exactly behind the last selected slot
    k = (src_h >= 0).sum(1)
    nd_p = torch.from_numpy((k * EVERY_N).astype(np.int32)).to(DEV)
    for plan in _plans(ops, nd, n):
        for mode in MODES:
            want = ops.l2norm_chunk(inp_p, 20, EVERY_N, C2, teacher_view=False, num_frames=nd_p if u8 else None, plan2=plan, **mode)[1]
            got = ops.l2norm_chunk_sel(inp, src, EVERY_N, C2, num_frames=nd if u8 else None, plan2=plan, **mode)
            assert _same(_live(got, plan, ops), _live(want, plan, ops)), (mode, plan is not None)
        if u8:
            want = ops.l2norm_chunk_int(inp_p, nd_p, 20, EVERY_N, C2, plan2=plan, teacher_view=False)[1]
            got = ops.l2norm_chunk_int_sel(inp, nd, src, EVERY_N, C2, plan2=plan)
            assert _same(_live(got, plan, ops), _live(want, plan, ops)), plan is not None


def test_gather_pad_rule_follows_the_source_frame(ops, frames):
    """A table may name a frame at or beyond num_frames (the selection never does): uint8 gives a zero row there, as -1 does."""
    q, _, n = frames[128]
    nd = torch.from_numpy(n).to(DEV)
    src = torch.full((B2, T2 // EVERY_N), -1, dtype=torch.int32, device=DEV)
    src[:, 0], src[:, 1], src[:, 2] = 40, 41, 299
    img = ops.l2norm_chunk_sel(torch.from_numpy(q).to(DEV), src, EVERY_N, C2, num_frames=nd).float()      # [6][C2 * B][F], slot j -> [j % 6][(j // 6) * B + b]
    assert (img[0, 2].abs().sum() > 0) and (img[1, 2] == 0).all() and (img[2, 2] == 0).all()            # video 2 has 41 frames
    assert (img[2, 0].abs().sum() > 0) and (img[3:] == 0).all()


# ---- 3. the graphs ------------------------------------------------------------------------------------------------------------------
GRAPH_KW = dict(every_n=10, feature_size=128, vocab_size=50, lstm_cells=64, device=DEV)


@pytest.mark.parametrize("precision,u8", [("bf16", False), ("high", True)])
@pytest.mark.parametrize("strategy", ["first", "middle", "last", "first_middle_last", "random"])
def test_eval_graph_equals_uniform_graph_on_rearranged_frames(precision, u8, strategy):
    from efficientvideoclassification_youtube8m_amd.distill import EvalGraph
    q, x, n, labels = mm.synthetic_batch(6, seed=3, feature_size=128, vocab_size=50, dtype=np.float32)
    n[0], n[1] = 300, 79
    host = q if u8 else x
    g = EvalGraph(6, student_only=True, precision=precision, student_sampling=strategy, sampling_seed=4, **GRAPH_KW)
    u = EvalGraph(6, student_only=True, precision=precision, **GRAPH_KW)
    u.restore(g.student.state_dict())
    nd, yd = torch.from_numpy(n).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV)
    out = g.step(torch.from_numpy(host).to(DEV), yd, nd, num_frames_host=n)
    pred, state = out["predictions"].clone(), out["student_state"].clone()
    src = g.last_frame_table.cpu().numpy()
    assert np.array_equal(src, ref.table(n, 300, 10, strategy, seed=4, draw=0, row0=0))
    # x': the selected frames on the uniform grid.  Slot j < k sits at frame j * every_n < n, inside the video (no padding); what x' holds
    # in the slots >= k is beyond the student's length k and is never read by its LSTMs.
    out_u = u.step(torch.from_numpy(ref.rearrange(host, src, 10)).to(DEV), yd, nd, num_frames_host=n)
    assert torch.equal(pred, out_u["predictions"]) and torch.equal(state, out_u["student_state"])
    assert torch.equal(out["num_frames"], out_u["num_frames"])
    plain = u.step(torch.from_numpy(host).to(DEV), yd, nd, num_frames_host=n)
    assert not torch.equal(pred, plain["predictions"])                             # and it is not the uniform student of x


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = tmp_path_factory.mktemp("frame_select") / "res.pt"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_frame_select_child.py"), str(out)],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = torch.load(str(out))
    print(res)
    assert res["deterministic"] == "1" and res["same_start"]
    return res


def test_teacher_is_untouched_by_the_students_frames(child):
    """teacher_student, one step under "last": the teacher's loss, outputs and updated weights are those of the uniform step."""
    assert child["table_last"] and child["student_differs"] and child["teacher_moved"]
    assert child["teacher_loss_equal"], child["teacher_loss"]
    assert child["teacher_pred_equal"] and child["teacher_weights_equal"]


def test_training_forward_equals_eval_graph(child):
    assert child["student_forward_equal"] and child["eval_teacher_equal"]


def test_student_only_step_equals_uniform_step_on_rearranged_frames(child):
    assert child["table_first"] and child["first_moved"] and child["first_is_not_uniform"]
    assert child["first_loss_equal"], child["first_loss"]
    assert child["first_pred_equal"] and child["first_weights_equal"]


def test_random_draws_follow_the_iteration(child):
    assert child["random_tables"] and child["random_redrawn"]


# ---- 4. the binaries ----------------------------------------------------------------------------------------------------------------
COMMON = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model",
          "HierarchicalLstmModel", "--gpu", "0", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64",
          "--every_n", "10", "--num_readers", "2"]


def test_binaries_with_student_sampling(tmp_path, ops):
    from efficientvideoclassification_youtube8m_amd import eval_finetune, inference, readers, train, train_convert_model, train_finetune
    from efficientvideoclassification_youtube8m_amd.distill import EvalGraph
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    data = tmp_path / "yt8m"
    readers.write_synthetic_frame_dataset(str(data), 2, 7, feature_sizes=(64, 64), min_frames=60, max_frames=310, seed=2, prefix="test")
    pattern = str(data / "test*.tfrecord")
    tdir = str(tmp_path / "model_train") + "/"
    synth = ["--synthetic_videos", "16", "--batch_size", "8", "--num_epochs", "1"]
    mid = ["--student_sampling", "middle"]
    try:
        FLAGS.reset()
        train.main(COMMON + mid + synth + ["--train_data_pattern", "synthetic", "--train_dir", tdir, "--start_new_model", "True"])
        sd = torch.load(train.latest_checkpoint(tdir))
        assert sd["student_sampling"] == "middle" and sd["global_step"] == 4
        FLAGS.reset()
        ck = train_convert_model.main(["--train_dir", tdir] + mid)
        assert torch.load(ck)["student_sampling"] == "middle"
        fdir = train_convert_model.finetune_dir(tdir)
        FLAGS.reset()
        train_finetune.main(COMMON + mid + synth + ["--train_data_pattern", "synthetic", "--train_dir", fdir, "--start_new_model", "False"])
        sdf = torch.load(train.latest_checkpoint(fdir))
        assert sdf["student_sampling"] == "middle" and sdf["global_step"] == 2
        FLAGS.reset()
        info = eval_finetune.main(COMMON + mid + ["--eval_data_pattern", "synthetic", "--synthetic_videos", "16", "--train_dir", fdir,
                                                  "--batch_size", "8", "--run_once", "True"])
        for key in ("avg_hit_at_one", "avg_perr", "avg_loss", "gap"):
            assert np.isfinite(info[key]), key
        assert info["epoch_id"] == 2 and info["avg_loss"] > 0

        def run(name, extra):
            out = str(tmp_path / name)
            FLAGS.reset()
            st = inference.main(COMMON + ["--input_data_pattern", pattern, "--output_file", out, "--batch_size", "5", "--top_k", "20"] + extra)
            assert st["videos"] == 14
            assert len(inference.read_prediction_file(out)) == 14
            return open(out, "rb").read()
        texts = {}
        for word in ("middle", "random", "uniform"):
            extra = ["--train_dir", fdir, "--student_sampling", word, "--student_sampling_seed", "3"]
            texts[word] = run(word + "1.csv", extra)
            assert texts[word] == run(word + "2.csv", extra)                          # byte-identical, also with random (draw 0)
        assert len({texts["middle"], texts["random"], texts["uniform"]}) == 3        # the flag wins over the checkpoint's word

        # two students of one checkpoint on the first and on the last frames, combined on the device
        got = run("ens.csv", ["--ensemble_dirs", fdir + "," + fdir, "--ensemble_sampling", "first,last", "--ensemble_mode", "max"])
        graphs = [EvalGraph(5, student_only=True, student_sampling=s, **dict(GRAPH_KW, vocab_size=4716)) for s in ("first", "last")]
        for g in graphs:
            g.restore(sdf)
        rd = readers.YT8MFrameFeatureReader(feature_names=["rgb", "audio"], feature_sizes=[64, 64], max_frames=300)
        want = [inference.HEADER]
        for ids, qd, yd, nd, nh in readers.get_input_evaluation_tensors(rd, sorted(glob.glob(pattern)), 5, 2, device=DEV, with_host_counts=True):
            preds = [g.step(qd, yd, nd, num_frames_host=nh)["predictions"] for g in graphs]
            assert not torch.equal(preds[0], preds[1])
            v, i = ops.ensemble_topk_rows(preds, 20, mode="max")
            want += list(inference.format_lines(ids, v.cpu().numpy(), i.cpu().numpy()))
        assert got.decode() == "".join(want)
    finally:
        FLAGS.reset()
