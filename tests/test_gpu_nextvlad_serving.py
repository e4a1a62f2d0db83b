"""Serving the NeXtVLAD family: evc_frames_gather_packed_sel and evc_scatter_rows exactly, NeXtVladEvalGraph against
the tower it wraps (bits) and against the float64 restatement tests/_nextvlad_serving_ref.py with and without compaction, a short last
batch without reallocation, and validate / inference / a mixed ensemble / a student -> teacher cascade end to end.  pytest -m gpu."""
import logging
import math
import re

import numpy as np
import pytest
import torch

import _nextvlad_serving_ref as sx
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
# the bound tests/test_gpu_nextvlad_distill.py::test_student_gradients_against_float64 holds the teacher's (every_n 1; measured 3.5e-3)
# and the student's (every_n 10; measured 1.9e-3) predictions to at this shape
PRED_BOUND = 5e-3
B4, F4, LAM, G4, K4, H4, RHO, V4, T4 = 32, 192, 2, 8, 24, 128, 2, 33, 300
EMPTY = (0, 7, 13, 22, 31)              # videos without a frame: the first, the last and three others


def _np(t):
    return t.detach().cpu().double().numpy()


# ---- the two kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [4, 192])
@pytest.mark.parametrize("bsel", [1, 27])
@pytest.mark.parametrize("every_n", [1, 7])
def test_gather_sel_is_the_gather_of_the_selected_videos(every_n, bsel, F):
    """evc_frames_gather_packed_sel on the unchanged batch against evc_frames_gather_packed on the batch gathered with index_select:
    torch.equal on the f32 and the bf16 rows - uint8 and f32 input, normalised or not, with and without the f32 output; rows R .. Rp
    zeros; everything behind Rp keeps the NaN it was prefilled with."""
    from efficientvideoclassification_youtube8m_amd import ops
    B, T = 32, 40
    rng = np.random.default_rng(every_n * 100 + bsel + F)
    n = rng.integers(1, T + 1, size=B).astype(np.int32)
    n[3], n[9] = T, 1
    sel = np.sort(rng.choice(B, size=bsel, replace=False)).astype(np.int32)
    if bsel > 1:
        sel[0], sel[-1] = 0, B - 1                                     # the first and the last video of the batch
    plan = ops.GridPlan(n[sel], every_n, T)
    R, Rp = plan.R, plan.Rp
    q = torch.from_numpy(rng.integers(0, 256, size=(B, T, F)).astype(np.uint8)).to(DEV)
    xf = torch.from_numpy(rng.standard_normal((B, T, F)).astype(np.float32)).to(DEV)
    nd, seld = torch.from_numpy(n).to(DEV), torch.from_numpy(sel).to(DEV)
    off = torch.from_numpy(plan.row_off).to(DEV)
    assert np.array_equal(ops.check_row_selection(sel, B), sel)
    for x in (q, xf):
        xs, ns = x.index_select(0, seld.long()).contiguous(), nd.index_select(0, seld.long()).contiguous()
        for normalize in (False, True):
            want = torch.full((Rp + 3, F), NAN, device=DEV)
            want_bf = torch.full((Rp + 3, F), NAN, dtype=torch.bfloat16, device=DEV)
            ops.frames_gather_packed(xs, ns, off, every_n, R, Rp, want, want_bf, normalize=normalize)
            for with_f32 in (True, False):
                got = torch.full((Rp + 3, F), NAN, device=DEV) if with_f32 else None
                got_bf = torch.full((Rp + 3, F), NAN, dtype=torch.bfloat16, device=DEV)
                ops.frames_gather_packed_sel(x, nd, off, seld, every_n, R, Rp, got, got_bf, normalize=normalize)
                torch.cuda.synchronize()
                what = (str(x.dtype), normalize, with_f32)
                assert torch.isfinite(want[:Rp]).all() and torch.equal(got_bf[:Rp], want_bf[:Rp]), what
                assert not got_bf[R:Rp].float().any() and torch.isnan(got_bf[Rp:].float()).all(), what
                if with_f32:
                    assert torch.equal(got[:Rp], want[:Rp]) and not got[R:Rp].any() and torch.isnan(got[Rp:]).all(), what
    assert not torch.equal(want[:R], torch.zeros_like(want[:R]))


@pytest.mark.parametrize("bsel", [1, 27, 32])
@pytest.mark.parametrize("V", [33, 4716])
def test_scatter_rows(V, bsel):
    """dst[sel[j]] = src[j]: the selected rows equal the source, every other row still holds its NaN - also from a source whose rows
    are a view of wider ones (row stride > V: the unaligned path)."""
    from efficientvideoclassification_youtube8m_amd import ops
    B = 32
    rng = np.random.default_rng(V + bsel)
    sel = np.sort(rng.choice(B, size=bsel, replace=False)).astype(np.int32)
    seld = torch.from_numpy(ops.check_row_selection(sel, B)).to(DEV)
    rest = np.setdiff1d(np.arange(B), sel)
    wide = torch.from_numpy(rng.standard_normal((bsel, V + 3)).astype(np.float32)).to(DEV)
    for src in (wide[:, :V].contiguous(), wide[:, 1:V + 1]):
        dst = torch.full((B, V), NAN, device=DEV)
        ops.scatter_rows(src, seld, dst)
        torch.cuda.synchronize()
        assert torch.equal(dst[torch.from_numpy(sel.astype(np.int64))], src)
        assert rest.size == 0 or torch.isnan(dst[torch.from_numpy(rest.astype(np.int64))]).all()


def test_new_entries_refuse_bad_shapes_and_null_operands():
    """EVC_ERR_BAD_SHAPE (-1) / EVC_ERR_BAD_ARG (-5) before any launch: the outputs keep what they held."""
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    B, T, F = 4, 8, 8
    x = torch.zeros((B, T, F), device=DEV)
    n = torch.full((B,), T, dtype=torch.int32, device=DEV)
    sel = torch.tensor([1, 3], dtype=torch.int32, device=DEV)
    off = torch.tensor([0, 8, 16], dtype=torch.int32, device=DEV)
    out = torch.full((32, F), 3.0, device=DEV)
    out_bf = torch.full((32, F), 3.0, dtype=torch.bfloat16, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()

    def gather(code, x_=x, n_=n, off_=off, sel_=sel, B_=B, bs=2, T_=T, F_=F, every_n=1, R=16, Rp=32, out_=out, bf=out_bf):
        with pytest.raises(_lib.EvcError, match=r"evc_frames_gather_packed_sel failed \(%d\)" % code):
            _lib.call("evc_frames_gather_packed_sel", p(x_), None, p(n_), p(off_), p(sel_), B_, bs, T_, F_, every_n, R, Rp, 0, p(out_), p(bf), 0)

    gather(-1, F_=6)
    gather(-1, bs=5)                                                   # more selected videos than the batch holds
    gather(-1, bs=0)
    gather(-1, every_n=0)
    gather(-1, R=17, Rp=32)                                            # R > Bsel * ceil(T / every_n)
    gather(-1, R=16, Rp=48)                                            # Rp - R >= 32
    gather(-5, sel_=None)
    gather(-5, off_=None)
    gather(-5, n_=None)
    gather(-5, out_=None, bf=None)
    gather(-5, x_=None)
    src, dst = torch.ones((2, 5), device=DEV), torch.full((4, 5), 3.0, device=DEV)

    def scatter(code, src_=src, sel_=sel, n_=2, rows=4, C=5, dst_=dst, ld_src=5, ld_dst=5):
        with pytest.raises(_lib.EvcError, match=r"evc_scatter_rows failed \(%d\)" % code):
            _lib.call("evc_scatter_rows", p(src_), ld_src, p(sel_), n_, rows, C, p(dst_), ld_dst, 0)

    scatter(-1, n_=5)
    scatter(-1, n_=-1)
    scatter(-1, C=0)
    scatter(-1, ld_dst=4)
    scatter(-1, ld_src=4)
    scatter(-5, sel_=None)
    scatter(-5, src_=None)
    scatter(-5, dst_=None)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((out_bf == 3.0).all()) and bool((dst == 3.0).all())
    with pytest.raises(ValueError, match="strictly ascending"):
        ops.check_row_selection([2, 1], 4)


# ---- the graph at the small shape of DESIGN.md 7.14 ---------------------------------------------------------------------------------------
_SHARED = {}
SIZES = dict(feature_size=F4, vocab_size=V4, max_frames=T4, cluster_size=K4, hidden_size=H4, groups=G4, expansion=LAM, gating_reduction=RHO,
             device=DEV)


def _perturb_moving(tw, rng):
    """(tests/test_gpu_nextvlad_distill.py's _perturb_moving)"""
    for k, v in tw.buffers.items():
        r = torch.from_numpy(rng.random(v.shape).astype(np.float32)).to(DEV)
        v.copy_(v * (1.0 + 0.1 * r) if k.endswith("variance") else v + 0.05 * (r - 0.5))


def _shared():
    """One checkpoint (teacher on every real frame in model/*, student on every 10th in model_student/*: scales, offsets and biases
    perturbed, moving statistics perturbed as _perturb_moving does), one batch with and without empty videos, and the float64
    predictions of both towers on both - made once."""
    if _SHARED:
        return _SHARED
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    rng = np.random.default_rng(B4 + K4)
    sd = {}
    for scope, every_n, seed in (("model", 1, 3), ("model_student", 10, 4)):
        tw = NeXtVladTower(B4, training=False, scope=scope, seed=seed, frames="grid", every_n=every_n, **SIZES)
        for k in tw.names:
            if k.endswith("/gamma") or k.endswith("/beta") or k in (tw.EB, tw.AB):
                tw.store.p(k).add_(torch.from_numpy(rng.standard_normal(tw.store.p(k).shape).astype(np.float32) * 0.2).to(DEV))
        tw.refresh_shadows()
        _perturb_moving(tw, rng)
        sd.update({k: v.cpu() for k, v in tw.state_dict().items()})
        del tw
    sd.update(global_step=4, nextvlad_frames="grid", every_n=10, teacher_every_n=1, student_sampling="uniform")
    q, x, n, labels = mm.synthetic_batch(B4, seed=B4, feature_size=F4, vocab_size=V4, dtype=np.float32)
    n = n.astype(np.int32)
    assert n.min() >= 120 and n.max() <= 300
    n_empty = n.copy()
    n_empty[list(EMPTY)] = 0
    xn = mm.l2_normalize(x.astype(np.float64), 2)
    ref = {}
    for scope, every_n in (("model", 1), ("model_student", 10)):
        P, M = sx.split_params(sd, scope)
        ref[scope, "full"] = sx.served_fwd(xn, n, every_n, P, M)
        ref[scope, "empty"] = sx.served_fwd(xn, n_empty, every_n, P, M)
    dev = (torch.from_numpy(q).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV))
    _SHARED.update(sd=sd, n=n, n_empty=n_empty, dev=dev, ref=ref)
    return _SHARED


def _graph(tower, compact, every_n=None, batch_size=B4, **kw):
    from efficientvideoclassification_youtube8m_amd.distill import NeXtVladEvalGraph
    every_n = every_n or (1 if tower == "teacher" else 10)
    g = NeXtVladEvalGraph(batch_size, tower=tower, every_n=every_n, teacher_every_n=1, compact=compact, **SIZES, **kw)
    g.restore(_shared()["sd"])
    return g


def _step(g, n, rows=None):
    sh = _shared()
    q, labels = sh["dev"]
    n = n if rows is None else n[:rows]
    q, labels = (q, labels) if rows is None else (q[:rows], labels[:rows])
    out = g.step(q, labels, torch.from_numpy(n).to(DEV), num_frames_host=n)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tower", ["teacher", "student"])
def test_graph_is_the_tower(tower):
    """No empty video: step() hands out the bits of NeXtVladTower(training=False).forward(is_training=False) on the same checkpoint,
    predictions and state, with compact on and off."""
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    sh = _shared()
    scope, every_n = ("model", 1) if tower == "teacher" else ("model_student", 10)
    tw = NeXtVladTower(B4, training=False, scope=scope, seed=99, frames="grid", every_n=every_n, **SIZES)
    tw.load_state_dict(sh["sd"])
    nd = torch.from_numpy(sh["n"]).to(DEV)
    want = tw.forward(sh["dev"][0], nd, num_frames_host=sh["n"], is_training=False).clone()
    want_state = tw.state.clone()
    for compact in (True, False):
        out = _step(_graph(tower, compact), sh["n"])
        assert out["predictions"].shape == (B4, V4) and torch.equal(out["predictions"], want)
        assert torch.equal(out[tower + "_state"], want_state)
        assert np.array_equal(out["num_frames"].numpy(), -(-sh["n"] // every_n))
        assert float(out["loss"]) > 0 and float(out["loss"]) == float(out["student_label_loss"])


def test_served_towers_against_float64():
    """The served teacher (every real frame) and student (every 10th) within the 5e-3 of the distillation test, with compact=True on
    the batch that has five empty videos (their rows: zeros, exactly) and with compact=False on the same batch and on the full one.
    Every figure is printed before the first assertion; the largest difference between compact on and off over the videos that have
    a frame goes into DESIGN.md 7.15 (bit equality is not asserted: the NT dispatch may depend on the row count).
    Measured on an MI355X: teacher 2.73e-3, student 2.92e-3 in all three runs (state 1.83e-2 / 1.55e-2); the rows of the empty videos
    with compact=False 1.44e-3 / 1.69e-3; compact on against off: 0 for both towers."""
    sh = _shared()
    missed, have = [], np.setdiff1d(np.arange(B4), EMPTY)
    for tower, scope in (("teacher", "model"), ("student", "model_student")):
        got = {}
        for compact, which in ((True, "empty"), (False, "empty"), (False, "full")):
            g = _graph(tower, compact)
            out = _step(g, sh["n_empty"] if which == "empty" else sh["n"])
            served = g.teacher if tower == "teacher" else g.student
            assert served.B == (B4 - len(EMPTY) if compact else B4) and served.cap == B4
            pred, state = _np(out["predictions"]), _np(out[tower + "_state"])
            want_pred, want_state = sh["ref"][scope, which]
            rows = have if which == "empty" else np.arange(B4)
            e = float(np.abs(pred[rows] - want_pred[rows]).max())
            print("%s compact=%s %s batch: predictions err %.2e (bound %.0e), state err %.2e"
                  % (tower, compact, which, e, PRED_BOUND, np.abs(state[rows] - want_state[rows]).max()))
            if not e < PRED_BOUND:
                missed.append((tower, compact, which, e))
            if compact:
                if pred[list(EMPTY)].any() or state[list(EMPTY)].any():
                    missed.append((tower, "rows of empty videos are not zero"))
            elif which == "empty":                                     # such a video runs behind the aggregation like any other
                e0 = float(np.abs(pred[list(EMPTY)] - want_pred[list(EMPTY)]).max())
                print("%s compact=False: rows of the empty videos err %.2e" % (tower, e0))
                if not e0 < PRED_BOUND:
                    missed.append((tower, "empty rows", e0))
            got[compact, which] = pred
        d = float(np.abs(got[True, "empty"][have] - got[False, "empty"][have]).max())
        print("%s: largest |compact on - compact off| over the videos with a frame: %.3e" % (tower, d))
        if not d < 2 * PRED_BOUND:                                     # (both lie within the bound of the same float64 value)
            missed.append((tower, "on / off", d))
    assert not missed, missed


def test_both_towers_report_the_state_loss():
    """tower='both' (validate): the student served, the teacher run too; student_state_loss is ops.rep_loss of the two states handed
    out, also on the batch with empty videos (their rows are zeros in both states and add nothing)."""
    from efficientvideoclassification_youtube8m_amd import ops
    sh = _shared()
    g = _graph("both", True)
    for n in (sh["n"], sh["n_empty"]):
        out = _step(g, n)
        assert set(out) >= {"predictions", "loss", "student_label_loss", "student_state", "teacher_state", "teacher_predictions",
                            "student_state_loss", "num_frames"}
        want = torch.zeros(1, device=DEV)
        ops.rep_loss(out["teacher_state"], out["student_state"], want)
        torch.cuda.synchronize()
        got = float(out["student_state_loss"])
        assert got > 0 and abs(got - float(want)) <= 1e-5 * abs(got), (got, float(want))
    single = _step(_graph("student", True), sh["n_empty"])
    assert torch.equal(single["predictions"], out["predictions"]) and torch.equal(single["student_state"], out["student_state"])


@pytest.mark.parametrize("compact", [True, False])
def test_short_last_batch_allocates_nothing(compact):
    """b = 19 after b = 32 on one graph: every buffer of the tower keeps its address, and the 19 videos stay within the bound."""
    sh = _shared()
    g = _graph("student", compact)
    tw = g.student
    _step(g, sh["n_empty"])
    names = ("r_bf", "xe", "xe_bf", "a", "Vv", "U", "Y_bf", "hid", "h_bf", "out", "row_off", "sel")
    before = {k: getattr(tw, k).data_ptr() for k in names}
    before.update(pred=tw.moe.pred.data_ptr(), x_bf=tw.moe.x_full.data_ptr())
    out = _step(g, sh["n_empty"], rows=19)
    after = {k: getattr(tw, k).data_ptr() for k in names}
    after.update(pred=tw.moe.pred.data_ptr(), x_bf=tw.moe.x_full.data_ptr())
    assert after == before and tw.cap == B4
    assert out["predictions"].shape == (19, V4) and out["student_state"].shape == (19, H4)
    have = np.array([b for b in range(19) if b not in EMPTY])
    want = sh["ref"]["model_student", "empty"][0]
    e = float(np.abs(_np(out["predictions"])[have] - want[have]).max())
    print("short batch compact=%s: predictions err %.2e (bound %.0e)" % (compact, e, PRED_BOUND))
    assert e < PRED_BOUND
    if compact:
        assert tw.B == len(have) and not out["predictions"][[0, 7, 13]].any()
    with pytest.raises(ValueError, match="a batch of 33 videos"):
        g.step(torch.zeros((33, T4, F4), device=DEV), torch.zeros((33, V4), dtype=torch.uint8, device=DEV),
               torch.ones(33, dtype=torch.int32, device=DEV))


# ---- the binaries, on checkpoints train.main wrote ---------------------------------------------------------------------------------------
NX = ["--nextvlad_cluster_size", "16", "--nextvlad_groups", "4", "--nextvlad_hidden_size", "128", "--nextvlad_gating_reduction", "2"]
FEATURES = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--gpu", "0"]
NXM = FEATURES + NX + ["--model", "NeXtVLADModel"]
HLM = FEATURES + NX + ["--model", "HierarchicalLstmModel", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64",
                       "--every_n", "10", "--num_readers", "1"]


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """A NeXtVLAD teacher trained 4 steps on every real frame, a --teacher_dir student trained 4 steps on every 10th, a small H-LSTM
    teacher trained 1 step, and a few records to predict."""
    from efficientvideoclassification_youtube8m_amd import readers, train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    root = tmp_path_factory.mktemp("nextvlad_serving")
    tdir, sdir, hdir = (str(root / d) + "/" for d in ("teacher", "student", "hlstm"))
    data = root / "yt8m"
    readers.write_synthetic_frame_dataset(str(data), 2, 11, feature_sizes=(64, 64), min_frames=60, max_frames=310, seed=1, prefix="test")
    feed = ["--train_data_pattern", "synthetic", "--batch_size", "16", "--nextvlad_frames", "grid", "--synthetic_videos", "64",
            "--num_epochs", "1", "--base_learning_rate", "0.01", "--start_new_model", "True"]
    try:
        FLAGS.reset()
        train.main(NXM + feed + ["--train_dir", tdir, "--every_n", "1"])
        FLAGS.reset()
        train.main(NXM + feed + ["--train_dir", sdir, "--every_n", "10", "--teacher_dir", tdir])
        FLAGS.reset()
        train.main(HLM + ["--train_data_pattern", str(data / "test*.tfrecord"), "--batch_size", "8", "--train_dir", hdir, "--max_steps", "1",
                          "--start_new_model", "True", "--teacher_only", "True"])
    finally:
        FLAGS.reset()
    return dict(tdir=tdir, sdir=sdir, hdir=hdir, records=str(data / "test*.tfrecord"), root=root)


def _fresh(train_dir, tower, args):
    """A fresh NeXtVladEvalGraph of one tower of train_dir's checkpoint at the sizes of the flags ``args`` set."""
    from efficientvideoclassification_youtube8m_amd import inference, train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.parse(args)
    ck = train.latest_checkpoint(train_dir)
    sd = torch.load(ck, map_location="cpu")
    towers = ("student", "teacher") if tower == "both" else (tower,)
    g = inference.nextvlad_graph(train.get_reader(), sd, tower, inference.nextvlad_every_n(sd, towers[0]), FLAGS.batch_size, DEV,
                                 teacher_every_n=inference.nextvlad_every_n(sd, "teacher"))
    g.restore(sd)
    return g


def test_validate_end_to_end(trained, caplog):
    """validate.main on the teacher's and on the student's directory (24 synthetic videos in batches of 16: a short last batch):
    Hit@1 / PERR / GAP / the per-class APs are exactly what eval_util computes on the host from the predictions of a fresh graph, the
    loss within float32 summation, the same numbers with --metrics_on_device True, and the student_loss it logs is the graph's."""
    from efficientvideoclassification_youtube8m_amd import eval_util, train, validate
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    try:
        for d, tower in ((trained["tdir"], "teacher"), (trained["sdir"], "both")):
            args = NXM + ["--train_dir", d, "--eval_data_pattern", "synthetic", "--synthetic_videos", "24", "--batch_size", "16",
                          "--run_once", "True", "--top_k", "20"]
            FLAGS.reset()
            caplog.clear()
            with caplog.at_level(logging.INFO):
                info = validate.main(args)
            logged = [float(m.group(1)) for m in (re.search(r"student_loss: ([0-9.]+) \|", r.getMessage()) for r in caplog.records) if m]
            FLAGS.reset()
            on_device = validate.main(args + ["--metrics_on_device", "True"])
            g = _fresh(d, tower, args)
            evl = eval_util.EvaluationMetrics(train.NUM_CLASSES, 20)
            state_losses = []
            for q, y, n, nh in train.synthetic_batches(16, 128, DEV, 24, 1, 4321):
                out = g.step(q, y, n, num_frames_host=nh)
                evl.accumulate(out["predictions"].cpu().numpy(), y.cpu().numpy().astype(np.float32), out["loss"].cpu().numpy())
                if tower == "both":
                    state_losses.append(float(out["student_state_loss"]))
            want = evl.get()
            assert info["epoch_id"] == 4
            for got in (info, on_device):
                for k in ("avg_hit_at_one", "avg_perr", "gap"):
                    assert got[k] == want[k], (d, k, got[k], want[k])
                assert np.array_equal(np.asarray(got["aps"]), np.asarray(want["aps"]))
                assert abs(got["avg_loss"] - want["avg_loss"]) <= 1e-5 * abs(want["avg_loss"])
            if tower == "both":
                assert len(logged) == 2 and all(abs(a - b) <= 1e-5 * abs(b) + 1e-6 for a, b in zip(logged, state_losses)), (logged, state_losses)
            else:
                assert not logged
    finally:
        FLAGS.reset()


def _selected(select):
    """The prediction file's text from select(q, labels, n, n_host) -> (values, indices), over inference's own batches."""
    import glob
    from efficientvideoclassification_youtube8m_amd import inference, readers, train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    text = [inference.HEADER]
    pipe = readers.get_input_evaluation_tensors(train.get_reader(), sorted(glob.glob(FLAGS.input_data_pattern)), batch_size=FLAGS.batch_size,
                                                num_readers=FLAGS.num_readers, device=DEV, with_host_counts=True)
    for ids, q, labels, n, nh in pipe:
        values, indices = select(q, labels, n, nh)
        text.extend(inference.format_lines(ids, values.cpu().numpy(), indices.cpu().numpy()))
    return "".join(text)


def test_inference_end_to_end(trained):
    """The prediction file is ops.topk_rows of a fresh graph's predictions, line for line; auto serves the student of a --teacher_dir
    checkpoint at its recorded grid, and --serve_tower teacher on that directory writes the teacher directory's file."""
    from efficientvideoclassification_youtube8m_amd import inference, ops
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    root = trained["root"]
    base = NXM + ["--input_data_pattern", trained["records"], "--batch_size", "8", "--top_k", "5", "--num_readers", "1"]
    try:
        files = {}
        for name, d, extra, member in (("student", trained["sdir"], [], ("student", 10)), ("teacher", trained["tdir"], [], ("teacher", 1)),
                                       ("teacher_of_student", trained["sdir"], ["--serve_tower", "teacher"], ("teacher", 1))):
            FLAGS.reset()
            out = str(root / (name + ".csv"))
            st = inference.main(base + extra + ["--train_dir", d, "--output_file", out])
            assert st["videos"] == 22 and st["batches"] == 3 and st["members"] == [(d,) + member]
            files[name] = open(out).read()
        assert files["teacher_of_student"] == files["teacher"] and files["student"] != files["teacher"]
        for name, d in (("student", trained["sdir"]), ("teacher", trained["tdir"])):
            args = base + ["--train_dir", d]
            g = _fresh(d, name, args)
            assert files[name] == _selected(lambda q, y, n, nh: ops.topk_rows(g.step(q, y, n, num_frames_host=nh)["predictions"], 5))
    finally:
        FLAGS.reset()


def test_mixed_ensemble_end_to_end(trained):
    """--ensemble_dirs with an H-LSTM and a NeXtVLAD member (each family from its own checkpoint): the file is
    ops.ensemble_topk_rows of the two members' own predictions."""
    from efficientvideoclassification_youtube8m_amd import inference, ops, train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    out = str(trained["root"] / "ensemble.csv")
    args = HLM + ["--input_data_pattern", trained["records"], "--batch_size", "8", "--top_k", "5", "--ensemble_mode", "mean",
                  "--ensemble_dirs", trained["hdir"] + "," + trained["sdir"], "--output_file", out]
    try:
        FLAGS.reset()
        st = inference.main(args)
        assert st["members"] == [(trained["hdir"], "teacher", 10), (trained["sdir"], "student", 10)] and st["videos"] == 22
        nx = _fresh(trained["sdir"], "student", args)
        hl = inference.build_graph(train.get_reader(), "teacher", 8, DEV)
        hl.restore(torch.load(train.latest_checkpoint(trained["hdir"]), map_location="cpu"))

        def combined(q, y, n, nh):
            preds = [hl.step(q, y, n, num_frames_host=nh)["predictions"], nx.step(q, y, n, num_frames_host=nh)["predictions"]]
            return ops.ensemble_topk_rows(preds, 5, mode="mean")
        assert open(out).read() == _selected(combined)
    finally:
        FLAGS.reset()


def test_student_teacher_cascade(trained):
    """--cascade_dirs student (10) -> teacher (1) of one distillation checkpoint with --cascade_fractions 0.25: every row carries the
    bits of the last stage that ran it, stage_rows / stage_frames are the host bookkeeping's, at most ceil(0.25 B) rows reach stage 1."""
    from efficientvideoclassification_youtube8m_amd import inference, train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    sdir, B = trained["sdir"], 16
    args = NXM + ["--batch_size", str(B), "--cascade_dirs", sdir + "," + sdir, "--cascade_towers", "student,teacher", "--cascade_fractions", "0.25"]
    try:
        FLAGS.reset()
        FLAGS.parse(args)
        spec = inference.cascade_spec()
        sds, members, _ = inference.load_members(spec)
        assert [m[1:] for m in members] == [("student", 10), ("teacher", 1)]
        graph = inference.build_cascade_graph(train.get_reader(), members, B, DEV, spec, sds)
        graph.restore(sds)
        assert graph.families == ["nextvlad", "nextvlad"]
        q, y, n, nh = next(iter(train.synthetic_batches(B, 128, DEV, B, 1, 77)))
        out = graph.step(q, y, n, num_frames_host=nh)
        torch.cuda.synchronize()
        nh = np.asarray(nh).reshape(-1)
        stage_of = out["stage_of"].cpu().numpy()
        escalated = stage_of == 1
        cap = math.ceil(0.25 * B)
        assert 0 < int(escalated.sum()) <= cap and set(stage_of.tolist()) <= {0, 1}
        assert out["stage_rows"] == [B, int(escalated.sum())]
        assert out["stage_frames"] == [sx.stage_frames(nh, None, 10, 300), sx.stage_frames(nh, escalated, 1, 300)]
        student = _fresh(sdir, "student", args).step(q, y, n, num_frames_host=nh)["predictions"].clone()
        masked = np.where(escalated, nh, 0)
        teacher = _fresh(sdir, "teacher", args).step(q, y, torch.from_numpy(masked.astype(np.int32)).to(DEV), num_frames_host=masked)["predictions"]
        merged = out["predictions"]
        assert torch.equal(merged[~torch.from_numpy(escalated)], student[~torch.from_numpy(escalated)])
        assert torch.equal(merged[torch.from_numpy(escalated)], teacher[torch.from_numpy(escalated)])
        assert not torch.equal(merged[torch.from_numpy(escalated)], student[torch.from_numpy(escalated)])
    finally:
        FLAGS.reset()
