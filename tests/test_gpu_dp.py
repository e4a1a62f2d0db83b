"""Data parallelism on the real kernels: two ranks (two processes sharing the one GPU of the test box, gloo
backend - RCCL refuses two ranks on one device) each train on half of a batch; the updated weights must equal
a single process training on the whole batch (loss scaling 1/world for the batch means, 1 for the L_PRED sum,
l2 term once, clip + Adam on the reduced gradient)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch
from oracle import model_math as mm
from efficientvideoclassification_youtube8m_amd.distill import DistillGraph
rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
torch.cuda.set_device(0)
FORCED = os.environ.get("EVC_DP_FORCE") == "1"          # a ONE-rank group whose collectives are all issued (backend from EVC_TEST_BACKEND: nccl = RCCL)
if world > 1 or FORCED:
    torch.distributed.init_process_group(os.environ.get("EVC_TEST_BACKEND", "gloo"), init_method="tcp://127.0.0.1:" + port, rank=rank, world_size=world)
GB, F, V = 8, 128, 200      # MoE gates [600][256]: 5 row tiles -> slabs of 384 / 216 rows on two ranks
q, x, n, labels = mm.synthetic_batch(GB, seed=21, feature_size=F, vocab_size=V, dtype=np.float32)
b = GB // world
sl = slice(rank * b, (rank + 1) * b)
PREC, H = os.environ.get("EVC_TEST_PRECISION", "bf16"), int(os.environ.get("EVC_TEST_CELLS", "64"))
g = DistillGraph(b, every_n=10, feature_size=F, vocab_size=V, lstm_cells=H, device="cuda:0", seed=3, precision=PREC)
xd = torch.from_numpy(q[sl]).cuda(); nd = torch.from_numpy(n[sl]).cuda(); yd = torch.from_numpy(labels[sl].astype(np.uint8)).cuda()
for it in range(2):
    o = g.step(xd, yd, nd, num_frames_host=n[sl])
rep = g.loss_report()
torch.cuda.synchronize()
if world > 1 and PREC == "bf16":
    # the fused data-parallel update leaves the f32 MoE weights / moments sharded by rows: reading them must fail loudly ...
    assert g.teacher.moe._stale and g.teacher.moe.slab[g.teacher.moe.GATES] == 384
    try:
        g.teacher.state_dict()
        raise SystemExit("state_dict() of a sharded tower did not raise")
    except RuntimeError:
        pass
g.consolidate()            # ... until every rank has gathered the slabs (collective; no-op on one rank)
if rank == 0:
    sd = {}
    sd.update({k: v.cpu() for k, v in g.teacher.state_dict().items()})
    sd.update({k: v.cpu() for k, v in g.student.state_dict().items()})
    sd["losses"] = rep
    sd["global_step"] = g.global_step
    sd["backend"] = torch.distributed.get_backend() if (world > 1 or FORCED) else None
    sd["dp_active"] = bool(g.dp)
    torch.save(sd, out)
if world > 1 or FORCED:
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
'''


def _run(world, out, port, env=None):
    code = WORKER % {"root": ROOT}
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), str(world), str(port), out], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, env=dict(os.environ, **(env or {}))) for r in range(world)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for pp in procs:
                pp.kill()
            raise
        logs.append(o.decode()[-2000:])
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)


@pytest.mark.parametrize("serial", ["0", "1"])
def test_two_rank_data_parallel_matches_single_process(tmp_path, serial):
    """serial = "1": EVC_DP_SERIAL_COMM - one communicator, every collective funnelled through one stream."""
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    _run(1, one, 29611)
    _run(2, two, 29612 + int(serial), env={"EVC_DP_SERIAL_COMM": serial})
    a, b = torch.load(one), torch.load(two)
    assert a["global_step"] == b["global_step"] == 4
    for k in ("label_loss", "student_loss_state", "pred_loss", "student_label_loss"):
        assert abs(a["losses"][k] - b["losses"][k]) <= 2e-3 * abs(a["losses"][k]) + 1e-6, (k, a["losses"], b["losses"])
    worst = 0.0
    for k, v in a.items():
        if torch.is_tensor(v):
            d = (v - b[k]).abs().max().item()
            # two Adam steps of lr 1e-3: an update is ~1e-3 per weight; the two runs may differ by summation order
            # (bf16 operands, f32 accumulation) - a few percent of one update at most
            worst = max(worst, d)
            assert d < 2e-4, (k, d)
    print("max weight difference single vs 2-rank:", worst)


def test_two_rank_data_parallel_in_high_precision(tmp_path):
    """precision = "high" under data parallelism (lstm_cells 128: the MoE head on its f16 + e4m3 operands, K = 512; the LSTM levels on
    their f16 K-extensions at these sizes): the MoE gradients are materialised and all-reduced (the fused sharded update is the bf16
    mode's), every operand image is rebuilt from the f32 masters after the update - two ranks on half a batch each must land on the
    single process's weights."""
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    env = {"EVC_TEST_PRECISION": "high", "EVC_TEST_CELLS": "128"}
    _run(1, one, 29651, env=env)
    _run(2, two, 29652, env=env)
    a, b = torch.load(one), torch.load(two)
    assert a["global_step"] == b["global_step"] == 4
    for k in ("label_loss", "student_loss_state", "pred_loss", "student_label_loss"):
        assert abs(a["losses"][k] - b["losses"][k]) <= 2e-3 * abs(a["losses"][k]) + 1e-6, (k, a["losses"], b["losses"])
    # (the single process updates the MoE weights with the fused kernel, the two ranks with materialised, all-reduced gradients: the same
    #  gradient to ~1e-6, but Adam's first steps move a weight by ~lr * sign(g), so an element whose gradient is within that of zero can
    #  land a good part of an update (1e-3) away - bounded by share and RMS, as in the bf16-payload test below)
    worst, report = 0.0, {}
    for k, v in a.items():
        if torch.is_tensor(v) and v.dtype == torch.float32 and v.numel() > 1:
            d = (v - b[k]).abs()
            worst = max(worst, d.max().item())
            far, rms = float((d > 2e-4).float().mean()), float(d.square().mean().sqrt())
            report[k.split("/", 1)[1]] = (round(far, 6), rms)
            assert d.max().item() < 2.5e-3 and far < 1e-3 and rms < 2e-5, (k, d.max().item(), far, rms)
    print("high precision, single vs 2-rank: max |dw| %.2e; (share > 2e-4, rms) per tensor: %s" % (worst, report))


def test_two_rank_bf16_gradient_payload_bounds_its_effect_on_the_update(tmp_path):
    """EVC_DP_GRAD_DTYPE=bf16: the LSTM gradient segments cross the fabric as bf16 (half the bytes: for the configurations whose
    step is shorter than their f32 all-reduce, cfg 5).  Each rank's gradient is rounded once (2^-9 relative) before the sum.
    What that does to the update, two iterations of Adam(1e-3) against the f32-payload run on the same two ranks: Adam's first
    steps move every weight by ~lr * sign(g), so an element whose summed gradient is smaller than the rounding of its two
    summands can flip and land a whole update (1e-3 per iteration) away - the MAX difference is therefore of the order of
    the update itself; the bound that means something is how many elements do that and the RMS: asserted < 2 % of the
    elements further than 2e-4 (the f32 two-rank tolerance) and an RMS difference below 15 % of one update (5 % / 20 % for the
    bias vectors, 256 elements each, where two or three flipped elements already show)."""
    f32, b16 = str(tmp_path / "f32.pt"), str(tmp_path / "bf16.pt")
    _run(2, f32, 29641)
    _run(2, b16, 29642, env={"EVC_DP_GRAD_DTYPE": "bf16"})
    a, b = torch.load(f32), torch.load(b16)
    assert a["global_step"] == b["global_step"] == 4
    for k in ("label_loss", "student_loss_state", "pred_loss", "student_label_loss"):
        assert abs(a["losses"][k] - b["losses"][k]) <= 2e-3 * abs(a["losses"][k]) + 1e-6, (k, a["losses"], b["losses"])
    worst, moved, report = 0.0, 0, {}
    for k, v in a.items():
        if torch.is_tensor(v) and v.dtype == torch.float32 and v.numel() > 1:
            d = (v - b[k]).abs()
            worst = max(worst, d.max().item())
            moved += int(d.max().item() > 0)
            far = float((d > 2e-4).float().mean())
            rms = float(d.square().mean().sqrt())
            report[k.split("/", 1)[1]] = (round(far, 5), rms)
            assert d.max().item() < 2.5e-3, (k, d.max().item())               # at most a flipped update in both iterations
            small = v.numel() < 10000
            assert far < (0.05 if small else 0.02) and rms < (2e-4 if small else 1.5e-4), (k, far, rms)
    assert moved > 0, "the bf16 payload changed nothing: the option did not reach the reducer"
    print("f32 vs bf16 gradient payload after two iterations: max |dw| %.2e; (share > 2e-4, rms) per tensor: %s" % (worst, report))


@pytest.mark.parametrize("route", ["factors", "reduce_scatter"])
def test_one_rank_rccl_group_runs_the_data_parallel_step(tmp_path, route):
    """The data-parallel graph on backend "nccl" (= RCCL) with ONE rank (EVC_DP_FORCE=1: every collective of the step is issued on the one-rank
    communicators - gradient all-reduces, factor all-gathers / gradient reduce-scatter, slab gathers, norm and loss sums): two iterations must
    land on the plain single-process step's losses and weights.  RCCL refuses two ranks per device and the test box has one GPU, so this is
    the only place where the suite loads RCCL and runs its kernels in the step's streams; the two-rank arithmetic is the gloo tests above."""
    one, rc = str(tmp_path / "one.pt"), str(tmp_path / "rccl.pt")
    _run(1, one, 29671)
    _run(1, rc, 29672 + (route == "factors"), env={"EVC_DP_FORCE": "1", "EVC_TEST_BACKEND": "nccl", "EVC_DP_MOE_ROUTE": route, "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    a, b = torch.load(one), torch.load(rc)
    assert a["backend"] is None and not a["dp_active"] and b["backend"] == "nccl" and b["dp_active"]
    assert a["global_step"] == b["global_step"] == 4
    for k in ("label_loss", "student_loss_state", "pred_loss", "student_label_loss"):
        assert abs(a["losses"][k] - b["losses"][k]) <= 2e-3 * abs(a["losses"][k]) + 1e-6, (k, a["losses"], b["losses"])
    for k, v in a.items():
        if torch.is_tensor(v) and v.dtype == torch.float32 and v.numel() > 1:
            d = (v - b[k]).abs()
            if route == "reduce_scatter" and "classifier/" in k and v.numel() > 10000:      # the gradient crosses as bf16: share / RMS bound (see below)
                assert d.max().item() < 2.5e-3 and float((d > 2e-4).float().mean()) < 0.02 and float(d.square().mean().sqrt()) < 1.5e-4, k
            else:
                assert d.max().item() < 2e-4, (k, d.max().item())


def test_two_rank_moe_gradient_exchange_routes(tmp_path):
    """The exchange that carries the MoE weight gradient under data parallelism is chosen by shape (MoeHead.dp_route, round 6): the factor
    all-gather of the fused update grows with the batch, the bf16 reduce-scatter of the locally formed gradient onto the owners' row slabs
    (MoeHead.sharded_update) is a constant of the model - cfg 5 (B = 1024 per rank, W = 8): 398 vs 169 MB per rank and step.  Both routes
    forced on the same two ranks (EVC_DP_MOE_ROUTE) and the single process: the same losses; the factor route within the f32 two-rank
    tolerance of the single process (test above); the reduce-scatter route rounds each rank's gradient to bf16 once before the sum, which
    is bounded the way the bf16 LSTM payload is - by the share of elements further than 2e-4 and the RMS, not by the maximum (Adam's first
    steps move every weight by ~lr * sign(g))."""
    one, fac, rs = str(tmp_path / "one.pt"), str(tmp_path / "fac.pt"), str(tmp_path / "rs.pt")
    _run(1, one, 29661)
    _run(2, fac, 29662, env={"EVC_DP_MOE_ROUTE": "factors"})
    _run(2, rs, 29663, env={"EVC_DP_MOE_ROUTE": "reduce_scatter"})
    a, f, r = torch.load(one), torch.load(fac), torch.load(rs)
    assert a["global_step"] == f["global_step"] == r["global_step"] == 4
    for k in ("label_loss", "student_loss_state", "pred_loss", "student_label_loss"):
        for other in (f, r):
            assert abs(a["losses"][k] - other["losses"][k]) <= 2e-3 * abs(a["losses"][k]) + 1e-6, (k, a["losses"], other["losses"])
    moved, report = 0, {}
    for k, v in a.items():
        if torch.is_tensor(v) and v.dtype == torch.float32 and v.numel() > 1:
            assert (v - f[k]).abs().max().item() < 2e-4, (k, "factors route vs single process")
            d = (v - r[k]).abs()
            if "classifier/" in k:
                moved += int((f[k] - r[k]).abs().max().item() > 0)
            far, rms = float((d > 2e-4).float().mean()), float(d.square().mean().sqrt())
            report[k.split("/", 1)[1]] = (round(far, 5), rms)
            small = v.numel() < 10000
            assert d.max().item() < 2.5e-3 and far < (0.05 if small else 0.02) and rms < (2e-4 if small else 1.5e-4), (k, d.max().item(), far, rms)
    assert moved > 0, "the forced route changed nothing in the MoE weights: the switch did not reach the update"
    print("reduce-scatter route vs single process, (share > 2e-4, rms) per tensor:", report)


def test_bench_multi_rank_path_runs(tmp_path):
    """bench.py launched the way the driver launches it for N > 1 (torch.distributed.run, one process per rank),
    here with two ranks sharing the GPU over gloo: rank 0 prints the one JSON line with whole-job throughput."""
    import json
    env = dict(os.environ, EVC_BENCH_SHARED_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29631", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "16", "--pool", "2", "--cpu_videos", "2", "--cpu_budget", "8", "--full"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 32 and d["value"] > 0 and d["scaling"] == "weak"
    # the N > 1 line is complete: the roofline of the dominant kernel AND the CPU leg, which rank 0 times after
    # destroy_process_group() - no peer sits in a collective meanwhile (here a 2-video sample: the leg itself is tests/test_cpu_host.py's)
    assert d["roofline"]["frac"] > 0 and d["roofline"]["bound"] == "mfma"
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] == "port" and "after destroy_process_group" in d["cpu_baseline"]["sample"]
    assert abs(d["value"] - 2 * 16 * 300 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert all(np.isfinite(v) for v in d["losses"].values())
    # the N > 1 line names the placement of the collectives and accounts for what they move (per step, rank 0)
    dp = d["dp"]
    assert dp["world"] == 2 and dp["attempt"] == 0 and dp["grad_dtype"] == "f32" and "two communicators" in dp["placement"]
    col = dp["collectives"]
    lstm_params = 17309696 + 29368320                                  # L1 + L2 kernels and biases of one tower
    assert abs(col["all_reduce_grad_f32"]["payload_mb_per_step"] - 2 * lstm_params * 4 / 1e6) < 0.5      # both towers, f32
    assert col["all_gather_slabs"]["calls_per_step"] == 4 and col["all_gather_factors"]["calls_per_step"] == 6
    assert dp["wire_mb_per_rank_per_step"] > 0 and dp["collective_event_ms_per_step"] > 0


def test_bench_gpus_2_without_a_launcher_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it: the (GPU-untouched) parent starts two rank supervisors itself and the
    line reports n_gpus = 2 - here with the two ranks sharing the GPU over gloo (EVC_BENCH_SHARED_GPU=1; RCCL refuses two ranks
    per device)."""
    import json
    env = dict(os.environ, EVC_BENCH_SHARED_GPU="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--global_batch", "32", "--pool", "2",
           "--no_cpu_baseline"]                                              # (strong-scaling form: 32 videos per step over the two ranks)
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 32 and d["config"]["parallelism"] == "dp2" and d["value"] > 0
    assert d["scaling"] == "strong" and "batch 16 x 300" in d["config"]["workload"]
    assert d["dp"]["world"] == 2 and d["dp"]["process_group"] == dict(d["dp"]["process_group"], backend="gloo", ranks=2, launched_by="bench.py --gpus N itself")
    assert d["ms_per_step_median"] > 0 and d["ms_per_step_max"] >= d["ms_per_step_median"] and isinstance(d["stall_suspected"], bool)


def test_train_main_two_ranks(tmp_path):
    """The product's train.py entry with two ranks (sharing the GPU over gloo, EVC_TRAIN_SHARED_GPU=1): the iteration
    count agreement, the collective loss report at the logging steps, the sharded MoE update and the consolidated
    checkpoint written by rank 0 must all line up - a rank-0-only collective would hang here."""
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29621", EVC_TRAIN_SHARED_GPU="1",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    args = [sys.executable, "-m", "efficientvideoclassification_youtube8m_amd.train", "--train_data_pattern", "synthetic",
            "--train_dir", str(tmp_path) + "/", "--frame_features", "True", "--feature_names", "rgb, audio",
            "--feature_sizes", "64, 64", "--model", "HierarchicalLstmModel", "--batch_size", "4", "--num_inputs_to_lstm", "20",
            "--lstm_layers", "2", "--lstm_cells", "64", "--num_epochs", "1", "--every_n", "10", "--synthetic_videos", "24",
            "--start_new_model", "True", "--max_steps", "3"]
    procs = [subprocess.Popen(args, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              cwd=ROOT) for r in range(2)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for pp in procs:
                pp.kill()
            raise
        logs.append(o.decode()[-3000:])
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    cks = [f for f in os.listdir(tmp_path) if f.startswith("model.ckpt-")]
    assert cks == ["model.ckpt-6.pt"], cks                  # 3 iterations x 2 global steps, written once (rank 0)
    sd = torch.load(str(tmp_path / cks[0]))
    assert sd["global_step"] == 6
    assert all(torch.isfinite(v).all() for v in sd.values() if torch.is_tensor(v))
    assert "training step 6" in logs[0] and "Teacher_Loss" in logs[0]


DBOF_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch
from oracle import model_math as mm
from efficientvideoclassification_youtube8m_amd.distill import SingleTowerGraph
from efficientvideoclassification_youtube8m_amd.towers import DbofTower, NetVladTower
rank, world, port, out, kind = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
torch.cuda.set_device(0)
if world > 1:
    torch.distributed.init_process_group("gloo", init_method="tcp://127.0.0.1:" + port, rank=rank, world_size=world)
GB, F, V, S = 16, 128, 60, 10
q, x, n, labels = mm.synthetic_batch(GB, seed=8, feature_size=F, vocab_size=V, dtype=np.float32)
u = np.random.default_rng(1).random((GB, S)).astype(np.float32)
b = GB // world
sl = slice(rank * b, (rank + 1) * b)
if kind == "dbof":
    tw = DbofTower(b, 300, F, V, iterations=S, cluster_size=256, hidden_size=64, device="cuda:0", seed=3)
else:
    S = 8                                             # (b * S must be a multiple of 32 on every rank: 8 x 8 = 64)
    u = np.random.default_rng(1).random((GB, S)).astype(np.float32)
    tw = NetVladTower(b, 300, F, V, iterations=S, cluster_size=64, hidden_size=64, device="cuda:0", seed=3)
rng = np.random.default_rng(4)
for k in tw.names:                                   # non-trivial BN scale / offset so that their gradients matter
    if k.endswith("/gamma") or k.endswith("/beta"):
        tw.store.p(k).add_(torch.from_numpy(rng.standard_normal(tw.store.p(k).shape).astype(np.float32) * 0.2).cuda())
g = SingleTowerGraph(tw, base_learning_rate=float(os.environ.get("EVC_TEST_LR", "1e-2")))
xd = torch.from_numpy(x[sl]).cuda(); nd = torch.from_numpy(n[sl]).cuda(); yd = torch.from_numpy(labels[sl].astype(np.uint8)).cuda()
ud = torch.from_numpy(u[sl]).cuda()
g.step(xd, yd, nd, uniform=ud, apply=False)
grads = {k: tw.store.g(k).clone().cpu() for k in tw.names}
for it in range(2):
    g.step(xd, yd, nd, uniform=ud)
torch.cuda.synchronize()
g.consolidate()            # the fused data-parallel MoE update leaves the f32 weights sharded by rows (collective; no-op on one rank)
if rank == 0:
    sd = {k: v.cpu() for k, v in tw.state_dict().items()}
    torch.save({"sd": sd, "grads": grads, "global_step": g.global_step}, out)
if world > 1:
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
'''


@pytest.mark.parametrize("kind", ["dbof", "netvlad", "dbof_rs"])
def test_dbof_two_ranks_match_single_process(tmp_path, kind):
    """DbofTower under data parallelism (SyncBN partial sums all-reduced, gradient all-reduce WITHOUT the batch-norm
    scale/offset segments, which are already global): gradients after one step and weights after two more equal the
    single-process run on the whole batch.  (A second all-reduce of dgamma/dbeta would double them: their per-tensor
    clipped Adam step would still look similar, so the gradients themselves are compared.)"""
    outs = []
    # "dbof_rs": the MoE gradient by bf16 reduce-scatter onto the owners' slabs (MoeHead.sharded_update; what cfg 4's shape picks at 8 ranks)
    rs = kind == "dbof_rs"
    env = dict(os.environ, EVC_DP_MOE_ROUTE="reduce_scatter", EVC_TEST_LR="1e-3") if rs else None      # (both runs, one and two ranks, at lr 1e-3)
    kind = "dbof" if rs else kind
    for world, port in ((1, 29641), (2, 29642)):
        out = str(tmp_path / ("w%d.pt" % world))
        code = DBOF_WORKER % {"root": ROOT}
        procs = [subprocess.Popen([sys.executable, "-c", code, str(r), str(world), str(port + (10 if kind == "netvlad" else (20 if rs else 0))), out, kind],
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env) for r in range(world)]
        logs = []
        for p in procs:
            try:
                o, _ = p.communicate(timeout=300)
            except subprocess.TimeoutExpired:
                for pp in procs:
                    pp.kill()
                raise
            logs.append(o.decode()[-2000:])
        assert all(p.returncode == 0 for p in procs), "\n".join(logs)
        outs.append(torch.load(out))
    a, b = outs
    assert a["global_step"] == b["global_step"] == 2
    for k, ga in a["grads"].items():
        gb = b["grads"][k]
        scale = ga.abs().max().item() + 1e-12
        assert (ga - gb).abs().max().item() < 2e-2 * scale + 1e-7, (k, (ga - gb).abs().max().item(), scale)
    # (two Adam steps at lr 1e-2 move a weight by up to 2e-2; an element whose gradient is ~0 can take steps of opposite
    # sign in the two runs - the gradient comparison above is the parity check, this one only bounds the drift)
    tol = 2e-3 if kind == "dbof" else 8e-3
    for k, v in a["sd"].items():
        d = (v - b["sd"][k]).abs()
        if rs:
            # each rank's MoE gradient is rounded to bf16 once before the sum: an element whose summed gradient is smaller than that rounding can
            # take Adam steps (lr = 1e-3 each here) of the other sign, and the second iteration of every OTHER tensor then sees slightly different
            # MoE weights - bounded by share and RMS (as the bf16 LSTM payload above), the maximum by a flipped update in both iterations
            if not v.dtype.is_floating_point or v.numel() < 2:
                continue
            far, rms = float((d > 2e-4).float().mean()), float(d.square().mean().sqrt())
            small = v.numel() < 10000
            # (the small tensors are the batch-norm scales / offsets and biases of a 64-unit toy tower: their SECOND gradient sees the few flipped MoE
            #  weights directly - measured 20 % of cluster_bn/beta further than 2e-4, rms 2.6e-4 = a quarter of one update; the matrices the
            #  reduce-scatter actually carries are held to the bf16-payload bound)
            assert d.max().item() < 2.5e-3 and far < (0.3 if small else 0.03) and rms < (6e-4 if small else 2e-4), (k, d.max().item(), far, rms)
            continue
        assert d.max().item() < tol, (k, d.max().item())
