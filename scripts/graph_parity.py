"""Bit parity of the graphs' steps between two trees (profiles/graph_refactor_parity.txt): every configuration runs 3 steps under
EVC_DETERMINISTIC=1 in a process of its own and prints one SHA-256 over every tensor of each step's `out`, loss_report() and every
tower's state_dict().  Public API only, so the same file runs on either tree; point both runs at one built library with EVC_LIB.

    python scripts/graph_parity.py [--root TREE]      every configuration, each under its own time limit; stops at the first failure
    python scripts/graph_parity.py --one NAME         one configuration, in this process
    ... --detail                                      also a short digest per tensor, to find where two trees part
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

B, F, V, H = 8, 128, 100, 128
KW = dict(feature_size=F, vocab_size=V, lstm_cells=H)
FRAMES = [300, 7, 295, 300, 120, 64, 299, 151]      # full length, one short video, counts that are no multiple of any every_n used

# name -> (graph, constructor arguments, what else differs: environment, attributes set after construction, uint8 input, apply)
CONFIGS = {
    "ts_default": ("distill", dict(mode="teacher_student"), {}),
    "ts_no_overlap": ("distill", dict(mode="teacher_student", overlap_towers=False), {}),
    "ts_student_early": ("distill", dict(mode="teacher_student"), dict(attrs=dict(student_forward_early=True))),
    "ts_defer_updates": ("distill", dict(mode="teacher_student"), dict(env=dict(EVC_DEFER_UPDATES="1"))),
    "ts_single_stream": ("distill", dict(mode="teacher_student"), dict(env=dict(EVC_SINGLE_STREAM="1"))),
    "ts_apply_later": ("distill", dict(mode="teacher_student"), dict(apply=False)),
    "ts_high_uint8": ("distill", dict(mode="teacher_student", precision="high"), dict(uint8=True)),
    "ts_random": ("distill", dict(mode="teacher_student", student_sampling="random", sampling_seed=3), {}),
    "teacher": ("distill", dict(mode="teacher"), {}),
    "student_last": ("distill", dict(mode="student", student_sampling="last"), {}),
    "serial_all": ("distill", dict(mode="serial"), {}),
    "serial_rep": ("distill", dict(mode="serial", distill_losses=("rep",)), {}),
    "serial_change": ("distill", dict(mode="serial", student_sampling="change"), {}),
    "serial_high": ("distill", dict(mode="serial", precision="high"), {}),
    "students_k1": ("students", dict(every_n=(10,)), {}),
    "students_k3": ("students", dict(every_n=(10, 30, 20), student_sampling=("uniform", "last", "segment_change"),
                                     distill_losses=(("rep", "pred", "ce"), ("rep",), ("pred", "ce")), sampling_seed=3), {}),
    "eval_both": ("eval", dict(), {}),
    "eval_student_only": ("eval", dict(student_only=True), {}),
    "eval_teacher_only": ("eval", dict(teacher_only=True), {}),
    "ensemble": ("ensemble", dict(members=[("teacher", 10), ("student", 10, "change")]), {}),
    "single_tower_dbof": ("dbof", dict(), {}),
}


DETAIL = False


def digest_of(h, v, path=""):
    import torch
    if isinstance(v, dict):
        for k in sorted(v):
            h.update(str(k).encode())
            digest_of(h, v[k], "%s/%s" % (path, k))
        return
    if isinstance(v, (list, tuple)):
        for i, e in enumerate(v):
            digest_of(h, e, "%s/%d" % (path, i))
        return
    raw = v.detach().cpu().reshape(-1).view(torch.uint8).numpy().tobytes() if isinstance(v, torch.Tensor) else json.dumps(v).encode()
    h.update(raw)
    if DETAIL:
        print("    %-60s %s" % (path, hashlib.sha256(raw).hexdigest()[:12]))


def run_one(name):
    kind, kw, extra = CONFIGS[name]
    os.environ["EVC_DETERMINISTIC"] = "1"
    os.environ.update(extra.get("env", {}))
    sys.path.insert(0, os.getcwd())               # the tree under test is the working directory
    import numpy as np
    import torch
    from efficientvideoclassification_youtube8m_amd import distill
    dev = "cuda:0"
    rng = np.random.default_rng(11)
    x = rng.standard_normal((B, 300, F)).astype(np.float32)
    if extra.get("uint8"):
        x = rng.integers(0, 256, (B, 300, F)).astype(np.uint8)
    n = np.asarray(FRAMES, dtype=np.int32)
    labels = (rng.random((B, V)) < 0.05).astype(np.uint8)
    xd, yd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(n).to(dev)
    towers, step_kw = [], dict(num_frames_host=n)
    if kind == "distill":
        g = distill.DistillGraph(B, every_n=10, device=dev, seed=5, **KW, **kw)
        towers = [g.teacher, g.student]
    elif kind == "students":
        g = distill.SerialStudentsGraph(B, device=dev, seed=5, **KW, **kw)
        towers = [g.teacher] + list(g.students)
    elif kind == "eval":
        g = distill.EvalGraph(B, every_n=10, device=dev, **KW, **kw)
        towers = [g.teacher, g.student]
    elif kind == "ensemble":
        g = distill.EnsembleGraph(B, device=dev, **KW, **kw)
        towers = [t for m in g.members for t in (m.teacher, m.student)]
    else:
        from efficientvideoclassification_youtube8m_amd.towers import DbofTower
        tower = DbofTower(B, 300, F, V, iterations=30, cluster_size=256, hidden_size=64, device=dev, seed=3)
        g = distill.SingleTowerGraph(tower)
        towers = [tower]
        step_kw = dict(uniform=torch.from_numpy(rng.random((B, 30)).astype(np.float32)).to(dev))
    for k, v in extra.get("attrs", {}).items():
        assert hasattr(g, k), k
        setattr(g, k, v)
    if "apply" in extra:
        step_kw["apply"] = extra["apply"]
    h = hashlib.sha256()
    for it in range(3):
        out = g.step(xd, yd, nd, **step_kw)
        torch.cuda.synchronize()
        digest_of(h, out, "step%d/out" % it)
        if extra.get("apply") is False:
            g.apply_gradients(B)
        if hasattr(g, "loss_report"):
            digest_of(h, g.loss_report(), "step%d/loss_report" % it)
    if hasattr(g, "flush"):
        g.flush()
    torch.cuda.synchronize()
    for i, tw in enumerate(towers):
        if tw is not None:
            digest_of(h, tw.state_dict(), "tower%d" % i)
    print("%-20s %s" % (name, h.hexdigest()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=sorted(CONFIGS))
    ap.add_argument("--root", default=os.getcwd(), help="the tree whose package is run (its working directory)")
    ap.add_argument("--limit", type=int, default=120, help="seconds per configuration")
    ap.add_argument("--detail", action="store_true")
    a = ap.parse_args()
    global DETAIL
    DETAIL = a.detail
    if a.one:
        return run_one(a.one)
    for name in CONFIGS:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", name] + ["--detail"] * a.detail, cwd=a.root)
        if r.returncode != 0:
            sys.exit("%s: exit status %d" % (name, r.returncode))


if __name__ == "__main__":
    main()
