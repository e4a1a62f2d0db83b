"""DbofModel and FrameLevelLogisticModel towers over the C-ABI kernels.

Reference: cs/frame_level_models.py:85-195 (DBoF, add_batch_norm=True,
sample_random_frames=True, pooling 'max', MoE head), cs/model_utils.py:39-83,
and cs/frame_level_models.py:50-83 (logistic over the mean frame).
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from .engine import BF16, F32, MoeHead, TowerBase


_reducers = {}


def _maybe_allreduce(t, group):
    """SUM of the f64 batch-norm partial sums over the ranks (SyncBN), in place; returns the world size.  Goes through a
    distill.GradReducer of the group like every other collective of a step: in stream order on the current stream by default,
    funnelled through the process-wide serial stream under EVC_DP_SERIAL_COMM=1 (so that mode really has ONE collective in
    flight at a time, SyncBN included), and counted in GradReducer.stats."""
    if torch.distributed.is_available() and torch.distributed.is_initialized() and \
            torch.distributed.get_world_size(group) > 1:
        from .distill import GradReducer                     # (distill imports this module's towers lazily too)
        red = _reducers.get(group)               # keyed by the group object itself (an id() can be reused after a group is destroyed)
        if red is None or red.pg is not group:
            red = _reducers[group] = GradReducer(group)
        red.all_reduce_small(t)
        return red.world
    return 1


class BatchNorm:
    """slim.batch_norm(center=True, scale=True): training uses biased batch
    moments (eps 1e-3) and updates the moving averages (decay 0.999); eval uses
    the moving averages.  Under data parallelism the f64 partial sums are
    all-reduced (SyncBN) so statistics equal the single-device global batch."""

    def __init__(self, tower, scope, C):
        self.tw, self.scope, self.C = tower, scope, C
        dev = tower.device
        self.mean = torch.zeros(C, dtype=F32, device=dev)
        self.var = torch.ones(C, dtype=F32, device=dev)
        self.ws = torch.zeros(2 * C, dtype=torch.float64, device=dev)
        tower.buffers[scope + "/moving_mean"] = torch.zeros(C, dtype=F32, device=dev)
        tower.buffers[scope + "/moving_variance"] = torch.ones(C, dtype=F32, device=dev)

    @staticmethod
    def shapes(scope, C):
        return OrderedDict([(scope + "/beta", (C,)), (scope + "/gamma", (C,))])

    def gamma(self):
        return self.tw.store.p(self.scope + "/gamma")

    def beta(self):
        return self.tw.store.p(self.scope + "/beta")

    def stats(self, x, R, is_training):
        """Sets self.mean/var for this batch (training) or from the moving averages."""
        tw = self.tw
        if not is_training:
            self.mean.copy_(tw.buffers[self.scope + "/moving_mean"])
            self.var.copy_(tw.buffers[self.scope + "/moving_variance"])
            self.R_total = R
            return
        ops.bn_stats_partial(x, R, self.C, self.ws)
        world = _maybe_allreduce(self.ws, tw.pg)
        self.R_total = R * world
        ops.bn_stats_finalize(self.ws, self.R_total, self.C, self.mean, self.var)
        ops.ema_update(tw.buffers[self.scope + "/moving_mean"], self.mean)
        ops.ema_update(tw.buffers[self.scope + "/moving_variance"], self.var)

    def backward(self, x, dy, R, relu6, argmax=None, S=1, dx_f32=None, dx_bf16=None, dy2=None):
        """dy2 (None or [R, C] f32): a second gradient on the layer's output, added to dy in front of the relu6 mask inside both
        passes (evc_bn_bwd_partial_add / _finalize_add); None keeps the plain entries' calls."""
        tw = self.tw
        if dy2 is not None:
            ops.bn_bwd_partial_add(x, dy, dy2, R, self.C, self.mean, self.var, self.gamma(), self.beta(), relu6, self.ws, argmax, S)
            _maybe_allreduce(self.ws, tw.pg)
            ops.bn_bwd_finalize_add(x, dy, dy2, R, self.R_total, self.C, self.mean, self.var, self.gamma(), self.beta(), relu6,
                                    self.ws, argmax, S, dx_f32, dx_bf16,
                                    tw.store.g(self.scope + "/gamma"), tw.store.g(self.scope + "/beta"))
            return
        ops.bn_bwd_partial(x, dy, R, self.C, self.mean, self.var, self.gamma(), self.beta(), relu6, self.ws, argmax, S)
        _maybe_allreduce(self.ws, tw.pg)
        ops.bn_bwd_finalize(x, dy, R, self.R_total, self.C, self.mean, self.var, self.gamma(), self.beta(), relu6,
                            self.ws, argmax, S, dx_f32, dx_bf16,
                            tw.store.g(self.scope + "/gamma"), tw.store.g(self.scope + "/beta"))


class DbofTower(TowerBase):
    """Deep Bag of Frames: sample S frames -> input_bn -> .Wc -> cluster_bn -> relu6 -> max over frames -> .Wh ->
    hidden1_bn -> relu6 -> MoE (cs/frame_level_models.py:108-195).

    The [B*S, clusters] activation (503 MB of f32 at B=512) never exists in f32: the cluster GEMM's epilogue
    (evc_dbof_cluster_pool_fwd) leaves the batch-norm column sums and, per (video, cluster), the frame that the
    max-pool will select (max of sign(gamma)*x: batch-norm with a fixed-sign scale and relu6 are monotone); training
    keeps the activation as bf16 for the backward pass, which rewrites it in place as d(activation).
    Backward: the gradient wrt the batch-normalised input (a second 290 GFLOP product in the reference graph, whose
    only consumers are input_bn's gamma/beta) is not formed: with G = dact^T . xhat,  dWc = gamma_in * G,
    dgamma_in = sum_c Wc * G,  dbeta_in = 0 (evc_dbof_wgrad_finish)."""

    CW, HW = "cluster_weights", "hidden1_weights"        # the reference's unnamed tf.Variable / Variable_1
    l2_names = (MoeHead.GATES, MoeHead.EXPERTS)
    # gradients that the batch-norm backward passes already leave summed over the ranks (SyncBN: all-reduced f64 sums): not
    # part of the gradient all-reduce.  (input_bn's come from the rank's own G = dact^T . xhat and ARE all-reduced.)
    global_grad_names = tuple("%s/%s" % (s, v) for s in ("cluster_bn", "hidden1_bn") for v in ("beta", "gamma"))
    takes_uniform_draw = True
    timing = None      # bench.py: set to a list to collect (start, end) events around the cluster GEMM launches

    def __init__(self, batch_size, max_frames=300, feature_size=1152, vocab_size=4716, iterations=30,
                 cluster_size=8192, hidden_size=1024, num_mixtures=2, device="cuda:0", training=True,
                 scope="model", seed=0, process_group=None):
        self.device, self.training, self.scope, self.pg = torch.device(device), training, scope, process_group
        self.T, self.F, self.V, self.S = max_frames, feature_size, vocab_size, iterations
        self.Cc, self.Hd, self.Mx = cluster_size, hidden_size, num_mixtures
        if feature_size % 64 or cluster_size % 64 or hidden_size % 64:
            raise ValueError("feature/cluster/hidden sizes must be multiples of 64 for the MFMA GEMM tiles")
        if iterations > 32:
            raise ValueError("iterations=%d: the fused cluster kernel holds at most 32 sampled frames per video" % iterations)
        shapes = OrderedDict()
        shapes.update(BatchNorm.shapes("input_bn", feature_size))
        shapes[self.CW] = (cluster_size, feature_size)               # stored transposed [C][F]
        shapes.update(BatchNorm.shapes("cluster_bn", cluster_size))
        shapes[self.HW] = (hidden_size, cluster_size)                # stored transposed [Hd][C]
        shapes.update(BatchNorm.shapes("hidden1_bn", hidden_size))
        shapes.update(MoeHead.shapes(hidden_size, vocab_size, num_mixtures))
        self.buffers = OrderedDict()
        self._setup_store(shapes)
        self.bn_in = BatchNorm(self, "input_bn", feature_size)
        self.bn_cl = BatchNorm(self, "cluster_bn", cluster_size)
        self.bn_h = BatchNorm(self, "hidden1_bn", hidden_size)
        self.moe = MoeHead(self, hidden_size, vocab_size, num_mixtures)
        self._init_params(seed)
        self._alloc(batch_size)

    def _init_params(self, seed):
        """cs/frame_level_models.py:145-147,169-171: random_normal(stddev=1/sqrt(fan_in));
        BN gamma=1, beta=0; MoE glorot-uniform / zero bias."""
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed)
        for k, shp in self.store.shapes.items():
            p = self.store.p(k)
            if k in (self.CW, self.HW):
                p.copy_(torch.randn(shp, generator=gen, dtype=F32) / math.sqrt(shp[1]))
            elif len(shp) == 2:
                lim = math.sqrt(6.0 / (shp[0] + shp[1]))
                p.copy_((torch.rand(shp, generator=gen, dtype=F32) * 2 - 1) * lim)
            elif k.endswith("/gamma"):
                p.fill_(1.0)
        self.refresh_shadows()

    def _alloc(self, B):
        dev, F, S, Cc, Hd = self.device, self.F, self.S, self.Cc, self.Hd
        self.B = B
        self.R = B * S                                               # sampled frames of this rank's batch
        self.Mp, self.P_in, self.P_cl = ops.dbof_workspace(B, S)     # rows of the padded frame layout / partial-sum rows
        Mp = self.Mp
        self.r = torch.empty((Mp, F), dtype=F32, device=dev)         # sampled, l2-normalised frames (only live slots are written / read)
        self.idx = torch.empty((B, S), dtype=torch.int32, device=dev)
        self.part_in = torch.empty((self.P_in, 2, F), dtype=F32, device=dev)
        self.r_bn = torch.empty((Mp, F), dtype=BF16, device=dev)
        self.part_cl = torch.empty((self.P_cl, 2, Cc), dtype=F32, device=dev)
        self.xsel = torch.empty((B, Cc), dtype=F32, device=dev)
        self.arg = torch.empty((B, Cc), dtype=torch.uint8, device=dev)
        self.Bk = ops.round_up(B, 32)                                # batch rows as a TN contraction length (zero rows pad)
        self.pooled = torch.empty((B, Cc), dtype=F32, device=dev)
        self.pooled_bf = torch.zeros((self.Bk, Cc), dtype=BF16, device=dev)
        self.hid = torch.empty((B, Hd), dtype=F32, device=dev)
        self.h6 = torch.empty((B, Hd), dtype=F32, device=dev)
        self.moe.alloc(B, self.training)
        if self.training:
            self.xhat = torch.empty((Mp, F), dtype=BF16, device=dev)
            self.act = torch.empty((Mp, Cc), dtype=BF16, device=dev)  # bf16 activation, rewritten in place as d(activation)
            self.dhid_bf = torch.zeros((self.Bk, Hd), dtype=BF16, device=dev)
            self.dpooled = torch.empty((B, Cc), dtype=F32, device=dev)
            self.nslab = self._pick_nslab(Cc, F, Mp)
            self.slabs = torch.empty((self.nslab, Cc, F), dtype=F32, device=dev)
            self.wgrad_ws = torch.empty(((Cc + 7) // 8, F), dtype=F32, device=dev)

    # "high" precision on f16 + e4m3 operands (both operands' roundings corrected behind the f16 stages of the same launches: ops.gemm_nt_f16_fp8,
    # ops.dbof_cluster_pool_fwd_f16fp8) when every contraction length is a multiple of 128; EVC_HIGH_FP8_LO=0 or other sizes: the
    # separate hi / lo shadows and three split-bf16 products per contraction (also what precision "split" means here).
    def _alloc_high_shadows(self):
        import os
        dims_ok = self.F % 128 == 0 and self.F >= 256 and self.Cc % 128 == 0 and self.Cc >= 512 and self.Hd % 128 == 0 and self.Hd >= 512
        if self.precision == "high" and dims_ok and os.environ.get("EVC_HIGH_FP8_LO", "1") != "0":
            self.shadow_lo, self.shadow_w16, self.shadow_w8 = {}, {}, {}
            for k in (self.CW, self.HW, MoeHead.GATES, MoeHead.EXPERTS):
                shp = self.store.shapes[k]
                self.shadow_w16[k] = torch.zeros(shp, dtype=ops.F16, device=self.device)
                self.shadow_w8[k] = torch.zeros((shp[0], 2 * shp[1]), dtype=torch.uint8, device=self.device)
        else:
            super()._alloc_high_shadows()

    def _fp8_exps(self, k):
        return ops.FP8_DBOF_CLUSTER if k == self.CW else ops.FP8_MOE

    def _refresh_high(self, k):
        if k in getattr(self, "shadow_w8", {}):
            e = self._fp8_exps(k)
            p = self.store.p(k)
            ops.cast_f16(p, self.shadow_w16[k])
            ops.cast_fp8_lo(p, self.shadow_w8[k], hi_cols=p.shape[1], scale_exp=e["w_lo_exp"], hi_exp=e["w_hi_exp"])
        else:
            super()._refresh_high(k)

    @staticmethod
    def _pick_nslab(M, N, K):
        """Split-K factor of the cluster-weight gradient G [M][N] = dact^T . xhat over K rows: its 256x256 tiles rarely
        fill the 256 CUs (cfg 4: 32 x 5 = 160), so K is cut into slabs that the finishing pass adds on the way.  Cost
        model: rounds of 256 workgroups x (1/nslab) of a full-K tile, plus writing and reading nslab f32 slabs."""
        tiles = -(-M // 256) * -(-N // 256)
        nk = K // 32
        t_tile = 2.0 * 256 * 256 * K / 3.9e12                       # a CU at ~40 % of its MFMA peak
        best, best_cost = 1, None
        for n in range(1, 9):
            per = -(-nk // n)
            if per * (n - 1) >= nk or per < 8:
                continue
            cost = -(-tiles * n // 256) * t_tile / n + (n * 2.0 * M * N * 4 / 5e12 if n > 1 else 0.0)
            if best_cost is None or cost < best_cost * 0.97:
                best, best_cost = n, cost
        return best

    def _bn_train_stats(self, bn, part, P, width):
        """Column partial sums -> batch statistics of the GLOBAL batch (SyncBN) + moving averages."""
        ops.bn_partials_reduce(part, P, width, bn.ws)
        world = _maybe_allreduce(bn.ws, self.pg)
        bn.R_total = self.R * world
        ops.bn_finalize_ema(bn.ws, bn.R_total, width, bn.mean, bn.var, self.buffers[bn.scope + "/moving_mean"],
                            self.buffers[bn.scope + "/moving_variance"])

    def forward(self, x, num_frames, uniform, normalize=True, is_training=True):
        """x [B,T,F] raw frames, float32 or uint8 as the reader delivers them (Dequantize is fused; normalize=True
        fuses tf.nn.l2_normalize of the sampled frames); uniform [B,S] f32 in [0,1): the tf.random_uniform draw of
        SampleRandomFrames, supplied by the caller so runs are reproducible."""
        B = x.shape[0]
        if B != self.B:
            self._alloc(B)
        F, S, Cc, Hd = self.F, self.S, self.Cc, self.Hd
        high = self.precision != "bf16"
        tape = self.training and is_training
        ops.dbof_gather(x, uniform, num_frames, self.r, self.idx, self.part_in if is_training else None, normalize=normalize)
        if is_training:
            self._bn_train_stats(self.bn_in, self.part_in, self.P_in, F)
        else:
            self.bn_in.stats(None, self.R, False)
        fp8 = high and self.CW in getattr(self, "shadow_w8", {})      # "high" on f16 + e4m3 operands (else: three split-bf16 products)
        if fp8 and (not hasattr(self, "r_rows") or self.r_rows.shape[0] != self.r_bn.shape[0]):
            self.r_rows = torch.empty((self.Mp, 2 * F), dtype=ops.F16, device=self.r_bn.device)
            self.pooled_rows = torch.empty((B, 2 * Cc), dtype=ops.F16, device=self.r_bn.device)
        if high and not fp8 and (not hasattr(self, "r_bn_lo") or self.r_bn_lo.shape != self.r_bn.shape):
            self.r_bn_lo = torch.empty_like(self.r_bn)
            self.pooled_lo = torch.zeros_like(self.pooled_bf)
        if fp8:
            ops.dbof_input_bn_apply_f16fp8(self.r, B, S, F, self.bn_in.mean, self.bn_in.var, self.bn_in.gamma(), self.bn_in.beta(), self.r_rows,
                                           self.xhat if tape else None)
        else:
            ops.dbof_input_bn_apply(self.r, B, S, F, self.bn_in.mean, self.bn_in.var, self.bn_in.gamma(), self.bn_in.beta(), self.r_bn,
                                    self.r_bn_lo if high else None, self.xhat if tape else None)
        if self.timing is not None:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        if fp8:
            ops.dbof_cluster_pool_fwd_f16fp8(self.r_rows, self.shadow_w16[self.CW], self.shadow_w8[self.CW], B, S, F, Cc, self.bn_cl.gamma(),
                                             self.xsel, self.arg, act=self.act if tape else None, part=self.part_cl if is_training else None)
        else:
            ops.dbof_cluster_pool_fwd(self.r_bn, self.shadow_fwd[self.CW], B, S, F, Cc, self.bn_cl.gamma(), self.xsel, self.arg,
                                      act=self.act if tape else None, part=self.part_cl if is_training else None,
                                      r_bn_lo=self.r_bn_lo if high else None, wT_lo=self.shadow_lo[self.CW] if high else None)
        if self.timing is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.timing.append((e0, e1))
        if is_training:
            self._bn_train_stats(self.bn_cl, self.part_cl, self.P_cl, Cc)
        else:
            self.bn_cl.stats(None, self.R, False)
        ops.dbof_pool_finish(self.xsel, B, Cc, self.bn_cl.mean, self.bn_cl.var, self.bn_cl.gamma(), self.bn_cl.beta(), self.pooled,
                             self.pooled_bf, self.pooled_lo if (high and not fp8) else None)
        if fp8:          # pooled in [0, 6] (relu6): the MoE head's scales fit (6 * 2^6 = 384 < 448)
            ops.cast_f16_fp8x(self.pooled, self.pooled_rows)
            ops.gemm_nt_f16_fp8(self.pooled_rows, self.shadow_w16[self.HW], self.shadow_w8[self.HW], B, Hd, Cc, self.hid)
        elif high:
            ops.gemm_nt_split(self.pooled_bf, self.pooled_lo, self.shadow_fwd[self.HW], self.shadow_lo[self.HW], B, Hd, Cc, self.hid)
        else:
            ops.gemm_nt(self.pooled_bf, self.shadow_fwd[self.HW], B, Hd, Cc, self.hid)
        self.bn_h.stats(self.hid, B, is_training)
        ops.bn_apply(self.hid, B, Hd, self.bn_h.mean, self.bn_h.var, self.bn_h.gamma(), self.bn_h.beta(), True,
                     y_f32=self.h6)
        self._taped = tape
        return self.moe.forward(self.h6)

    def grad_stages(self):
        """Variable names in the order their gradients become final during backward(): (moe, hidden, cluster)."""
        moe = [MoeHead.GATES, MoeHead.EXPERTS, MoeHead.EBIAS]
        hidden = [self.HW, "hidden1_bn/beta", "hidden1_bn/gamma"]
        cluster = [k for k in self.names if k not in moe and k not in hidden]
        return moe, hidden, cluster

    def backward(self, dpred, on_moe_grads_ready=None, moe_weight_grads=True, on_stage=None):
        """moe_weight_grads=False: the two MoE weight gradients are not materialised (MoeHead.fused_update recomputes
        them from the factors inside the clip + Adam pass).  on_stage(i): called when the gradients of grad_stages()[i]
        are final (a data-parallel caller starts that stage's all-reduce there, under the rest of the backward pass)."""
        assert self.training and self._taped, "backward needs a training-mode forward"
        B, F, S, Cc, Hd = self.B, self.F, self.S, self.Cc, self.Hd
        st = self.store
        dh6 = self.moe.backward(dpred, weight_grads=moe_weight_grads)
        if on_moe_grads_ready is not None:
            on_moe_grads_ready()
        if on_stage is not None:
            on_stage(0)
        self.bn_h.backward(self.hid, dh6, B, True, dx_bf16=self.dhid_bf)
        # hidden1 weights: dWh^T [Hd][C] = dhid^T . pooled (TN over the batch rows); dpooled = dhid . Wh^T
        ops.gemm_tn(self.dhid_bf, self.pooled_bf, Hd, Cc, self.Bk, st.g(self.HW))
        if on_stage is not None:
            on_stage(1)
        ops.gemm_nt(self.dhid_bf, self.shadow_bwd[self.HW], B, Cc, Hd, self.dpooled)
        # max-pool routing + relu6 mask + cluster_bn backward: the two batch sums need only the [B][C] selected entries
        bn = self.bn_cl
        ops.bn_bwd_partial(self.xsel, self.dpooled, B, Cc, bn.mean, bn.var, bn.gamma(), bn.beta(), True, bn.ws)
        _maybe_allreduce(bn.ws, self.pg)
        ops.dbof_dact(self.act, self.dpooled, self.pooled, self.arg, bn.mean, bn.var, bn.gamma(), bn.ws, bn.R_total, B, S, Cc,
                      dgamma=st.g("cluster_bn/gamma"), dbeta=st.g("cluster_bn/beta"))
        # G = dact^T . xhat in split-K slabs, then cluster weights / input_bn gradients from G
        ops.gemm_tn_slabs(self.act, self.xhat, Cc, F, self.Mp, self.slabs, self.nslab)
        ops.dbof_wgrad_finish(self.slabs, self.nslab, Cc, F, st.p(self.CW), self.bn_in.gamma(), st.g(self.CW),
                              st.g("input_bn/gamma"), st.g("input_bn/beta"), part_ws=self.wgrad_ws)
        if on_stage is not None:
            on_stage(2)

    @property
    def pred(self):
        return self.moe.pred


class DbofGenericTower(TowerBase):
    """DbofModel with the flag values NO launcher of the reference selects (cs/frame_level_models.py:108-195): any combination of
    --dbof_pooling_method max | average (cs/model_utils.py:75-78), --dbof_add_batch_norm True | False (cluster_biases /
    hidden1_biases instead of the three slim.batch_norm, :158-161,181-185) and --sample_random_frames True | False
    (SampleRandomSequence, cs/model_utils.py:11-36).  The default combination runs on DbofTower (fused cluster kernel); this tower
    is the plain chain on the library's generic kernels - one launch per graph op group, the [B*S, clusters] activation in f32 -
    written for parity, not for speed.  ('none' pooling: FramePooling returns [B*S, C], so the predictions have B*S rows against B
    label rows: the reference's graph does not train with it - refused by DbofModel.create_model.)
    Precision (round 5): "high" = "split" here - the cluster, hidden and MoE products as split-bf16 (hi.hi + hi.lo + lo.hi, f32-operand
    accuracy: three launches per contraction on separate hi / lo shadows, TowerBase's default layout), so that these branches too have a
    mode inside north_star's 1e-3; the backward products stay bf16 as in every mode."""

    CW, CB, HW, HB = "cluster_weights", "cluster_biases", "hidden1_weights", "hidden1_biases"
    takes_uniform_draw = True
    l2_names = (MoeHead.GATES, MoeHead.EXPERTS)

    def __init__(self, batch_size, max_frames=300, feature_size=1152, vocab_size=4716, iterations=30, cluster_size=8192,
                 hidden_size=1024, num_mixtures=2, device="cuda:0", training=True, scope="model", seed=0, process_group=None,
                 pooling="max", add_batch_norm=True, random_frames=True):
        if pooling not in ("max", "average"):
            raise ValueError("Unrecognized pooling method: %s" % pooling)                  # cs/model_utils.py:83
        self.device, self.training, self.scope, self.pg = torch.device(device), training, scope, process_group
        self.T, self.F, self.V, self.S = max_frames, feature_size, vocab_size, iterations
        self.Cc, self.Hd, self.Mx = cluster_size, hidden_size, num_mixtures
        self.pooling, self.bn, self.random_frames = pooling, bool(add_batch_norm), bool(random_frames)
        if feature_size % 64 or cluster_size % 64 or hidden_size % 64:
            raise ValueError("feature/cluster/hidden sizes must be multiples of 64 for the MFMA GEMM tiles")
        F, Cc, Hd = feature_size, cluster_size, hidden_size
        shapes = OrderedDict()
        if self.bn:
            shapes.update(BatchNorm.shapes("input_bn", F))
        shapes[self.CW] = (Cc, F)                                    # stored transposed [C][F]
        if self.bn:
            shapes.update(BatchNorm.shapes("cluster_bn", Cc))
        else:
            shapes[self.CB] = (Cc,)
        shapes[self.HW] = (Hd, Cc)
        if self.bn:
            shapes.update(BatchNorm.shapes("hidden1_bn", Hd))
        else:
            shapes[self.HB] = (Hd,)
        shapes.update(MoeHead.shapes(Hd, vocab_size, num_mixtures))
        self.buffers = OrderedDict()
        self._setup_store(shapes)
        if self.bn:
            self.bn_in, self.bn_cl, self.bn_h = BatchNorm(self, "input_bn", F), BatchNorm(self, "cluster_bn", Cc), BatchNorm(self, "hidden1_bn", Hd)
        # batch-norm gradients leave BatchNorm.backward already summed over the ranks (all-reduced f64 sums)
        self.global_grad_names = tuple("%s/%s" % (s_, v) for s_ in ("input_bn", "cluster_bn", "hidden1_bn") for v in ("beta", "gamma")) if self.bn else ()
        self.moe = MoeHead(self, Hd, vocab_size, num_mixtures)
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed)
        for k, shp in self.store.shapes.items():          # cs/frame_level_models.py:145-147,158-160,169-171,182-184
            p = self.store.p(k)
            if k in (self.CW, self.HW):
                p.copy_(torch.randn(shp, generator=gen, dtype=F32) / math.sqrt(shp[1]))
            elif k == self.CB:
                p.copy_(torch.randn(shp, generator=gen, dtype=F32) / math.sqrt(F))
            elif k == self.HB:
                p.copy_(torch.randn(shp, generator=gen, dtype=F32) * 0.01)
            elif len(shp) == 2:
                lim = math.sqrt(6.0 / (shp[0] + shp[1]))
                p.copy_((torch.rand(shp, generator=gen, dtype=F32) * 2 - 1) * lim)
            elif k.endswith("/gamma"):
                p.fill_(1.0)
        self.refresh_shadows()
        self._alloc(batch_size)

    def _alloc(self, B):
        dev, F, S, Cc, Hd = self.device, self.F, self.S, self.Cc, self.Hd
        self.B, self.R = B, B * S
        R = self.R
        if self.training and R % 32:
            raise ValueError("batch_size x iterations = %d must be a multiple of 32 (row count of the TN weight-gradient products)" % R)
        self.Bk = ops.round_up(B, 32)
        self.r = torch.empty((R, F), dtype=F32, device=dev)
        self.idx = torch.empty((B, S), dtype=torch.int32, device=dev)
        self.r_bn = torch.empty((R, F), dtype=BF16, device=dev)
        self.act = torch.empty((R, Cc), dtype=F32, device=dev)      # pre-activation (before cluster_bn, or with its bias)
        self.a6 = torch.empty((R, Cc), dtype=F32, device=dev)
        self.arg = torch.empty((B, Cc), dtype=torch.int32, device=dev)
        self.pooled = torch.empty((B, Cc), dtype=F32, device=dev)
        self.pooled_bf = torch.zeros((self.Bk, Cc), dtype=BF16, device=dev)
        self.hid = torch.empty((B, Hd), dtype=F32, device=dev)
        self.h6 = torch.empty((B, Hd), dtype=F32, device=dev)
        self.moe.alloc(B, self.training)
        if self.training:
            self.dhid_bf = torch.zeros((self.Bk, Hd), dtype=BF16, device=dev)
            self.dpooled = torch.empty((B, Cc), dtype=F32, device=dev)
            self.dy = torch.empty((R, Cc), dtype=F32, device=dev)
            self.dact_bf = torch.empty((R, Cc), dtype=BF16, device=dev)
            self.dx = torch.empty((R, F), dtype=F32, device=dev)

    def forward(self, x, num_frames, uniform, normalize=True, is_training=True):
        """x [B,T,F] float32 or uint8; uniform: [B,S] f32 in [0,1) (SampleRandomFrames) or [B] / [B,1] (SampleRandomSequence)."""
        B = x.shape[0]
        if B != self.B:
            self._alloc(B)
        F, S, Cc, Hd, R, st = self.F, self.S, self.Cc, self.Hd, self.R, self.store
        if self.random_frames:
            ops.sample_frames_gather(x, uniform, num_frames, self.r, self.idx, normalize=normalize)
        else:
            u1 = uniform.reshape(B, -1)[:, 0].contiguous()
            ops.sample_sequence_gather(x, u1, num_frames, S, self.r, self.idx, normalize=normalize)
        hp = self.precision != "bf16"              # split-bf16 forward products (the operands' low-order halves in r_lo / pooled_lo / shadow_lo)
        if hp and (not hasattr(self, "r_lo") or self.r_lo.shape != self.r_bn.shape):
            self.r_f32 = torch.empty((R, F), dtype=F32, device=x.device)
            self.r_lo = torch.empty_like(self.r_bn)
            self.pooled_lo = torch.zeros_like(self.pooled_bf)

        def product(a_hi, a_lo, a_f32, k, M, N, K, out, bias=None):
            if hp:
                ops.cast_bf16_split(a_f32, a_hi[:M], a_lo[:M])
                ops.gemm_nt_split(a_hi, a_lo, self.shadow_fwd[k], self.shadow_lo[k], M, N, K, out, bias=bias)
            else:
                ops.gemm_nt(a_hi, self.shadow_fwd[k], M, N, K, out, bias=bias)
        if self.bn:
            bi, bc, bh = self.bn_in, self.bn_cl, self.bn_h
            bi.stats(self.r, R, is_training)
            ops.bn_apply(self.r, R, F, bi.mean, bi.var, bi.gamma(), bi.beta(), False, y_f32=self.r_f32 if hp else None, y_bf16=self.r_bn)
            product(self.r_bn, self.r_lo if hp else None, self.r_f32 if hp else None, self.CW, R, Cc, F, self.act)
            bc.stats(self.act, R, is_training)
            ops.bn_apply(self.act, R, Cc, bc.mean, bc.var, bc.gamma(), bc.beta(), True, y_f32=self.a6)
        else:
            ops.cast_bf16(self.r, self.r_bn)
            product(self.r_bn, self.r_lo if hp else None, self.r, self.CW, R, Cc, F, self.act, bias=st.p(self.CB))
            ops.relu6_fwd(self.act, y_f32=self.a6)
        if self.pooling == "max":
            ops.framepool_max_fwd(self.a6, B, S, Cc, self.pooled, self.pooled_bf, self.arg)
        else:
            ops.framepool_mean_fwd(self.a6, B, S, Cc, self.pooled, self.pooled_bf)
        if self.bn:
            product(self.pooled_bf, self.pooled_lo if hp else None, self.pooled, self.HW, B, Hd, Cc, self.hid)
            bh.stats(self.hid, B, is_training)
            ops.bn_apply(self.hid, B, Hd, bh.mean, bh.var, bh.gamma(), bh.beta(), True, y_f32=self.h6)
        else:
            product(self.pooled_bf, self.pooled_lo if hp else None, self.pooled, self.HW, B, Hd, Cc, self.hid, bias=st.p(self.HB))
            ops.relu6_fwd(self.hid, y_f32=self.h6)
        self._taped = self.training and is_training
        return self.moe.forward(self.h6)

    def grad_stages(self):
        moe = [MoeHead.GATES, MoeHead.EXPERTS, MoeHead.EBIAS]
        hidden = [k for k in (self.HW, self.HB, "hidden1_bn/beta", "hidden1_bn/gamma") if k in self.names]
        return moe, hidden, [k for k in self.names if k not in moe and k not in hidden]

    def backward(self, dpred, on_moe_grads_ready=None, moe_weight_grads=True, on_stage=None):
        assert self.training and self._taped, "backward needs a training-mode forward"
        B, F, S, Cc, Hd, R, st = self.B, self.F, self.S, self.Cc, self.Hd, self.R, self.store
        dh6 = self.moe.backward(dpred, weight_grads=moe_weight_grads)
        if on_moe_grads_ready is not None:
            on_moe_grads_ready()
        if on_stage is not None:
            on_stage(0)
        if self.bn:
            self.bn_h.backward(self.hid, dh6, B, True, dx_bf16=self.dhid_bf)
        else:
            ops.relu6_bwd(self.hid, dh6, dx_bf16=self.dhid_bf[:B])
            ops.colsum_bf16(self.dhid_bf, self.Bk, Hd, st.g(self.HB))
        ops.gemm_tn(self.dhid_bf, self.pooled_bf, Hd, Cc, self.Bk, st.g(self.HW))          # dWh^T [Hd][C]
        if on_stage is not None:
            on_stage(1)
        ops.gemm_nt(self.dhid_bf, self.shadow_bwd[self.HW], B, Cc, Hd, self.dpooled)
        if self.pooling == "max":
            ops.framepool_max_bwd(self.dpooled, self.arg, B, S, Cc, self.dy)
        else:
            ops.framepool_mean_bwd(self.dpooled, B, S, Cc, self.dy)
        if self.bn:
            self.bn_cl.backward(self.act, self.dy, R, True, dx_bf16=self.dact_bf)
        else:
            ops.relu6_bwd(self.act, self.dy, dx_bf16=self.dact_bf)
            ops.colsum_bf16(self.dact_bf, R, Cc, st.g(self.CB))
        ops.gemm_tn(self.dact_bf, self.r_bn, Cc, F, R, st.g(self.CW))                        # dWc^T [C][F]
        if self.bn:
            ops.gemm_nt(self.dact_bf, self.shadow_bwd[self.CW], R, F, Cc, self.dx)
            self.bn_in.backward(self.r, self.dx, R, False)
        if on_stage is not None:
            on_stage(2)

    @property
    def pred(self):
        return self.moe.pred


class VladTower(TowerBase):
    """What the two VLAD towers (NetVLAD, NeXtVLAD) share: the check of a checkpoint's shapes, the row bookkeeping of both frame modes, the
    packed layout of grid mode and the views of a forward-only grid tower that serves fewer videos than it was allocated for.  A family
    names itself in FAMILY / MODEL / FLAG (the prefix of its flags) and NOT_A_CHECKPOINT (vlad_graphs.check_vlad_checkpoint's clause)."""

    PRECISIONS = ("bf16",)             # no split-bf16 forward (set_precision refuses anything else)
    FRAME_MODES = ("sampled", "grid")
    takes_uniform_draw = property(lambda self: self.frames != "grid")

    @classmethod
    def checkpoint_shapes(cls, *sizes, **kw):
        """What state_dict() holds for these size flags, without the scope prefix: every variable in its TF layout (2-D weights
        [in][out]) and the batch norms' moving statistics.  For checking a checkpoint against the flags before a tower is built.
        Keywords are variable_shapes' (NetVLAD: gating=True, with the context gate's names)."""
        out = OrderedDict()
        for k, shp in cls.variable_shapes(*sizes, **kw).items():
            out[k] = tuple(reversed(shp)) if len(shp) == 2 else tuple(shp)
            if k.endswith("/gamma"):
                for v in ("moving_mean", "moving_variance"):
                    out[k[:-len("gamma")] + v] = tuple(shp)
        return out

    def _alloc_rows(self, B, with_sel=False):
        """The bookkeeping in front of _alloc's buffer list; returns the rows of the row buffers.  Grid mode: every row buffer once, for
        every video at full length - a batch uses its first R (Rp in the TN products) rows -, and row_off with its two pinned staging
        buffers (with_sel: the same for sel, a served subset of the batch's videos)."""
        dev = self.device
        if self.frames == "grid":
            self.B, self.R, self.Rp, self.plan = B, 0, 0, None
            R = ops.grid_capacity(B, self.T, self.every_n)
            self.row_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
            self._row_off_host = [torch.zeros(B + 1, dtype=torch.int32).pin_memory() for _ in range(2)]
            if with_sel:
                self.sel = torch.zeros(B, dtype=torch.int32, device=dev)
                self._sel_host = [torch.zeros(B, dtype=torch.int32).pin_memory() for _ in range(2)]
            self._row_off_done = [None, None]
            self._uploads = 0
        else:
            self.B, self.R = B, B * self.S
            if self.training and self.R % 32:
                raise ValueError("batch_size x iterations = %d must be a multiple of 32 (row count of the TN weight-gradient products)" % self.R)
            R = self.R
        self.cap = B                                                 # videos the buffers hold (forward-only grid towers serve B <= cap)
        self.Bk = ops.round_up(B, 32)
        return R

    def _fit_batch(self, B):
        """A batch of B videos: a forward-only grid tower keeps the buffers it allocated when they hold it, every other case allocates."""
        if B != self.B:
            if self.frames == "grid" and not self.training and B <= self.cap:
                self.B = B
            else:
                self._alloc(B)

    def _plan_grid_rows(self, num_frames, num_frames_host, sel=None, select=False):
        """Grid mode: this batch's packed layout from the HOST frame counts (launch sizes and offsets without a device sync); row_off goes
        up through one of two pinned buffers, reused only once its earlier copy has completed.  sel (int32 numpy, accepted by
        ops.check_row_selection): the layout of those videos alone, and sel itself goes up the same way.  select: the counts of a
        source-frame table (ops.SelectPlan) in place of the grid's."""
        if num_frames_host is None:
            num_frames_host = num_frames.cpu().numpy()       # an explicit device sync: callers that have the counts on the host pass them
        if sel is not None:
            num_frames_host = np.asarray(num_frames_host).reshape(-1)[sel]
        plan = (ops.SelectPlan if select else ops.GridPlan)(num_frames_host, self.every_n, self.T)
        if plan.B != self.B:
            raise ValueError("num_frames_host holds %d videos, the batch %d" % (plan.B, self.B))
        if plan.R == 0:
            raise ValueError("%s_frames grid: no video of the batch has a frame" % self.FLAG)
        slot = self._uploads % 2
        self._uploads += 1
        if self._row_off_done[slot] is not None:
            self._row_off_done[slot].synchronize()
        B = plan.B
        self._row_off_host[slot][:B + 1].copy_(torch.from_numpy(plan.row_off))
        self.row_off[:B + 1].copy_(self._row_off_host[slot][:B + 1], non_blocking=True)
        if sel is not None:
            self._sel_host[slot][:B].copy_(torch.from_numpy(sel))
            self.sel[:B].copy_(self._sel_host[slot][:B], non_blocking=True)
        ev = self._row_off_done[slot] = torch.cuda.Event()
        ev.record()
        self.plan, self.R, self.Rp = plan, plan.R, plan.Rp
        return plan

    def _live(self, t):
        """The rows of a [cap, .] buffer that belong to this batch."""
        return t if self.B == self.cap else t[:self.B]

    pred = property(lambda self: self._live(self.moe.pred))
    rowsum = property(lambda self: self._live(self.moe.rowsum))


def check_grid_frames(tower_cls, frames, every_n, max_frames, model, world, precision):
    """What --nextvlad_frames / --netvlad_frames grid refuse with --every_n, the model, the ranks and --precision, as ValueErrors that name
    the family's flag; touches no device."""
    flag, name = tower_cls.FLAG + "_frames", tower_cls.FAMILY
    if model is not None and model != tower_cls.MODEL:
        raise ValueError("%s grid is built for --model %s, not %s" % (flag, tower_cls.MODEL, model))
    if every_n < 1 or every_n > max_frames:
        raise ValueError("%s grid: --every_n %d must lie in 1 .. --max_num_frames %d" % (flag, every_n, max_frames))
    if world > 1:
        raise ValueError("%s grid refuses a process group of %d ranks: ragged ranks hold different row counts and the "
                         "batch-norm statistics assume equal ones; data parallelism is not built for this mode" % (flag, world))
    if precision != "bf16":
        raise ValueError("%s grid: --precision %s is refused, the %s tower has no such forward mode (bf16 only)" % (flag, precision, name))


class NetVladTower(VladTower):
    """NetVLAD aggregation tower - an EXTENSION: the reference announces NetVLAD / NeXtVLAD teacher-student variants
    (README.md:126-127) but ships empty stubs (cs/frame_level_models.py:341-355), so there is no reference math; the
    definition is oracle/model_math.py::netvlad_fwd ("Learnable pooling with Context Gating" NetVLAD in the frame of the
    DBoF tower): sample S frames -> input_bn -> .Wc -> cluster_bn -> softmax over K clusters -> V[k] = sum_s a[s,k] (x_s - c2[k])
    -> intra-normalise -> l2-normalise -> .Wh -> hidden1_bn -> relu6 -> MoE.
    GEMM-shaped parts on the library's NT / TN kernels, the f32 pieces in csrc/evc_netvlad.hip.  V / Y are kept
    cluster-major [B][K][F]; hidden1_weights' TF row order f*K + k is restored in state_dict().

    frames="grid" (DESIGN.md 7.18): instead of S drawn frames, video b contributes the frames j * every_n < min(n_b, T) - every real
    frame at every_n = 1, the fewer-frames student's grid above - as a ragged list of rows packed back to back (ops.GridPlan), with
    no limit on the rows of a video; padding frames are never computed.  The two batch-norms in front of the aggregation take their
    statistics over the R live rows, the aggregation runs on evc_netvlad_aggregate_packed_fwd / _bwd.  Same weights and checkpoint
    names: a tower of either mode loads the other's checkpoint.  A forward-only grid tower (training=False) keeps no gradient store
    or moments, runs on the moving statistics and serves batches of up to batch_size videos in the buffers it allocated; its gather and
    input_bn are one launch (evc_frames_gather_packed_bn).  `state` is h6 = relu6(hidden1_bn(hid)), what the MoE head
    reads; backward(dstate=...) adds a gradient on it in front of that relu6's mask (serial distillation's L_REP).

    gating=True (--netvlad_gating): the paper's context gate between the hidden layer and the classifier, in both frame modes:
    gl = bf16(h6) . gating_weights, state = h6 * sigmoid(gating_bn(gl)); the MoE head reads `state`, and so does L_REP.  Five more variables
    (gating_weights [H, H] and gating_bn's four), stored after hidden1_bn's; none is in l2_names.  The gate is evc_bn_gate_fwd and
    evc_bn_gate_bwd_partial / _finalize (fused_gate = False: the chain of older entries they replace, the same bits).  In the backward pass
    the head's gradient and dstate meet inside the gate, and hidden1_bn receives the gate's two gradients on h6 (the direct one and the one
    through gating_weights) as its dy / dy2.  One rank only.  Off, the tower has no such variable and issues the launches it always did.

    sampling (grid mode): a word of ops.STUDENT_SAMPLING / STUDENT_SAMPLING_SCORED.  Off "uniform" video b contributes the
    k_b = trunc(n_b / T * (T // every_n)) frames the word selects (ops.SelectPlan: the H-LSTM student's count, at most the grid's) - their
    table built on the device per batch (kept as last_frame_table), one gather that reads it (evc_frames_gather_packed_tab), everything
    behind the gather unchanged.  "random" draws from (sampling_seed, draw, row0 + b), forward's arguments."""

    FAMILY, MODEL, FLAG, NOT_A_CHECKPOINT = "NetVLAD", "NetVLADModel", "--netvlad", "not a NetVLADModel checkpoint"
    fused_input_pass = True           # forward-only grid towers: evc_frames_gather_packed_bn (False: the two launches, for A/B timing)
    fused_gate = True                 # gating: evc_bn_gate_fwd / _bwd_* (False: bn_apply, nextvlad_gate_*, bn_bwd_* one after another; same bits)

    CW, C2, HW, GW = "cluster_weights", "cluster_weights2", "hidden1_weights", "gating_weights"
    l2_names = (MoeHead.GATES, MoeHead.EXPERTS)
    # all three batch-norms go through BatchNorm.backward: their gamma/beta gradients are global (all-reduced f64 sums)
    # (a tower with the gate adds gating_bn's pair to its own copy)
    global_grad_names = tuple("%s/%s" % (s_, v) for s_ in ("input_bn", "cluster_bn", "hidden1_bn") for v in ("beta", "gamma"))

    def __init__(self, batch_size, max_frames=300, feature_size=1152, vocab_size=4716, iterations=30, cluster_size=64,
                 hidden_size=1024, num_mixtures=2, device="cuda:0", training=True, scope="model", seed=0, process_group=None,
                 frames="sampled", every_n=1, sampling="uniform", sampling_seed=0, gating=False):
        world = 1
        if process_group is not None and torch.distributed.is_available() and torch.distributed.is_initialized():
            world = torch.distributed.get_world_size(process_group)
        check_netvlad_frames(frames, every_n, max_frames, world=world, sampling=sampling)   # (before the device is touched)
        check_netvlad_gating(gating, world)
        self.gating = bool(gating)
        self.frames, self.every_n = frames, int(every_n)
        self.sampling, self.sampling_seed = sampling, int(sampling_seed)
        self.last_frame_table = None       # the source-frame table of the last batch (sampling != "uniform"), for tests and diagnostics
        self.device, self.training, self.scope, self.pg = torch.device(device), training, scope, process_group
        self.T, self.F, self.V, self.S = max_frames, feature_size, vocab_size, iterations
        self.Kc, self.Hd, self.Mx = cluster_size, hidden_size, num_mixtures
        if feature_size % 64 or cluster_size % 64 or hidden_size % 64:
            raise ValueError("feature / cluster / hidden sizes must be multiples of 64 for the MFMA GEMM tiles")
        if frames == "sampled" and iterations > 64:                  # (grid mode does not read iterations)
            raise ValueError("iterations=%d: the aggregation kernel holds at most 64 sampled frames per video" % iterations)
        F, K, H = feature_size, cluster_size, hidden_size
        shapes = self.variable_shapes(F, vocab_size, K, H, num_mixtures, gating=self.gating)
        self.buffers = OrderedDict()
        self._setup_store(shapes)
        self.bn_in = BatchNorm(self, "input_bn", F)
        self.bn_cl = BatchNorm(self, "cluster_bn", K)
        self.bn_h = BatchNorm(self, "hidden1_bn", H)
        if self.gating:
            self.bn_g = BatchNorm(self, "gating_bn", H)
            self.global_grad_names = type(self).global_grad_names + ("gating_bn/beta", "gating_bn/gamma")
        self.moe = MoeHead(self, H, vocab_size, num_mixtures)
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed)
        for k, shp in self.store.shapes.items():
            p = self.store.p(k)
            if k in (self.CW, self.C2):
                p.copy_(torch.randn(shp, generator=gen, dtype=F32) / math.sqrt(F))
            elif k == self.HW:
                p.copy_(torch.randn(shp, generator=gen, dtype=F32) / math.sqrt(K))
            elif k == self.GW:
                continue                                             # drawn behind every other variable, below
            elif len(shp) == 2:
                lim = math.sqrt(6.0 / (shp[0] + shp[1]))
                p.copy_((torch.rand(shp, generator=gen, dtype=F32) * 2 - 1) * lim)
            elif k.endswith("/gamma"):
                p.fill_(1.0)
        if self.gating:                                              # (after the others: the draws of a tower without the gate keep their values)
            self.store.p(self.GW).copy_(torch.randn((H, H), generator=gen, dtype=F32) / math.sqrt(H))
        self.refresh_shadows()
        if not training and frames == "grid":
            self.store.drop_training_state()                         # forward only: the masters alone
        self._alloc(batch_size)

    @classmethod
    def variable_shapes(cls, feature_size, vocab_size, cluster_size, hidden_size, num_mixtures, gating=False):
        """The trainable variables and their INTERNAL shapes, in store order, from the size flags alone (no device).  gating: with the
        context gate's variables behind hidden1_bn's."""
        F, K, H = feature_size, cluster_size, hidden_size
        shapes = OrderedDict()
        shapes.update(BatchNorm.shapes("input_bn", F))
        shapes[cls.CW] = (K, F)                                      # stored transposed [K][F]
        shapes.update(BatchNorm.shapes("cluster_bn", K))
        shapes[cls.C2] = (K, F)                                      # centres, stored [K][F] (tf: [1, F, K])
        shapes[cls.HW] = (H, K * F)                                  # stored transposed, columns cluster-major (k*F + f)
        shapes.update(BatchNorm.shapes("hidden1_bn", H))
        if gating:
            shapes[cls.GW] = (H, H)                                  # stored transposed [out][in]
            shapes.update(BatchNorm.shapes("gating_bn", H))
        shapes.update(MoeHead.shapes(H, vocab_size, num_mixtures))
        return shapes

    # hidden1_weights: TF layout [F*K, H] with row f*K + k  <->  internal [H][k*F + f]
    def state_dict(self):
        out = super().state_dict()
        key = "%s/%s" % (self.scope, self.HW)
        w = out[key]                                                 # [K*F (k-major), H]
        out[key] = w.view(self.Kc, self.F, self.Hd).permute(1, 0, 2).reshape(self.F * self.Kc, self.Hd).contiguous()
        return out

    def load_state_dict(self, sd, prefix=None):
        prefix = self.scope if prefix is None else prefix
        key = "%s/%s" % (prefix, self.HW)
        if key not in sd:
            raise KeyError("NetVladTower.load_state_dict: %r is not in the checkpoint (scope prefix %r; it holds e.g. %s)"
                           % (key, prefix, sorted(sd)[:3]))
        sd = dict(sd)
        sd[key] = sd[key].view(self.F, self.Kc, self.Hd).permute(1, 0, 2).reshape(self.Kc * self.F, self.Hd).contiguous()
        super().load_state_dict(sd, prefix)

    def _alloc(self, B):
        dev, F, S, K, H = self.device, self.F, self.S, self.Kc, self.Hd
        grid = self.frames == "grid"
        R = self._alloc_rows(B)          # (grid: the bf16 operands of the TN products start as zeros; their rows R .. Rp are zeroed again at every step)
        self.r = torch.empty((R, F), dtype=F32, device=dev)
        if not grid:
            self.idx = torch.empty((B, S), dtype=torch.int32, device=dev)
        self.r_bn = torch.zeros((R, F), dtype=BF16, device=dev) if grid else torch.empty((R, F), dtype=BF16, device=dev)
        self.act = torch.empty((R, K), dtype=F32, device=dev)
        self.a = torch.empty((R, K), dtype=F32, device=dev)
        self.asum = torch.empty((B, K), dtype=F32, device=dev)
        self.Vv = torch.empty((B, K, F), dtype=F32, device=dev)
        self.n1 = torch.empty((B, K), dtype=F32, device=dev)
        self.n2 = torch.empty((B,), dtype=F32, device=dev)
        self.Y_bf = torch.zeros((self.Bk, K * F), dtype=BF16, device=dev)
        self.hid = torch.empty((B, H), dtype=F32, device=dev)
        self.h6 = torch.empty((B, H), dtype=F32, device=dev)
        if self.gating:
            self.h6_bf = torch.zeros((self.Bk, H), dtype=BF16, device=dev)      # (rows B .. Bk stay zeros: an operand of the TN product)
            self.gl = torch.empty((B, H), dtype=F32, device=dev)
            self.gated = torch.empty((B, H), dtype=F32, device=dev)
            if not self.fused_gate:
                self.gn = torch.empty((B, H), dtype=F32, device=dev)
        self.moe.alloc(B, self.training)
        if self.training:
            if self.gating:
                self.dgl_bf = torch.zeros((self.Bk, H), dtype=BF16, device=dev)
                self.dh6_via = torch.empty((B, H), dtype=F32, device=dev)
                self.dh6_direct = torch.empty((B, H), dtype=F32, device=dev)
                if not self.fused_gate:
                    self.dgn = torch.empty((B, H), dtype=F32, device=dev)
            self.dhid_bf = torch.zeros((self.Bk, H), dtype=BF16, device=dev)
            self.dY = torch.empty((B, K * F), dtype=F32, device=dev)
            self.dV = torch.empty((B, K, F), dtype=F32, device=dev)
            self.da = torch.empty((R, K), dtype=F32, device=dev)
            self.dz = torch.empty((R, K), dtype=F32, device=dev)
            self.dx = torch.empty((R, F), dtype=F32, device=dev)
            self.dact_bf = torch.zeros((R, K), dtype=BF16, device=dev) if grid else torch.empty((R, K), dtype=BF16, device=dev)
            if grid:
                self.agg_ws = torch.empty(ops.netvlad_aggregate_packed_bwd_ws(B, K, F), dtype=F32, device=dev)

    def forward(self, x, num_frames, uniform=None, normalize=True, is_training=True, num_frames_host=None, keys=None, draw=0, row0=0):
        """x [B,T,F] float32 or uint8 raw frames; uniform [B,S] f32 in [0,1): the frame-sampling draw (sampled mode; not read in grid
        mode, which takes num_frames_host, the frame counts on the host, instead).  A forward-only grid tower keeps the buffers it
        allocated: a batch of fewer videos uses their first rows.  keys / draw / row0 are read by a tower with a sampling word alone:
        the batch's ops.frame_change_keys where the caller has them (scored words), and the draw of "random"."""
        B = x.shape[0]
        grid = self.frames == "grid"
        select = grid and self.sampling != "uniform"
        self._fit_batch(B)
        F, S, K, H = self.F, self.S, self.Kc, self.Hd
        st, bi, bc = self.store, self.bn_in, self.bn_cl
        if self.precision != "bf16":
            raise NotImplementedError("NetVladTower has no split-bf16 mode")
        if grid:
            if x.shape[1] != self.T:
                raise ValueError("the batch holds %d frames per video, the tower was built for max_frames=%d" % (x.shape[1], self.T))
            if select:
                # the frames of a --student_sampling word: their table on this stream, as distill.input_views builds it
                if self.sampling in ops.STUDENT_SAMPLING_SCORED:
                    if keys is None:
                        keys = ops.frame_change_keys(x, num_frames)
                    src = ops.student_frame_select_scored(num_frames, keys, self.T, self.every_n, self.sampling)
                else:
                    src = ops.student_frame_select(num_frames, self.T, self.every_n, self.sampling, seed=self.sampling_seed, draw=draw, row0=row0)
                self.last_frame_table = src
            plan = self._plan_grid_rows(num_frames, num_frames_host, select=select)
            R, Rp = plan.R, plan.Rp
            row_off = self.row_off[:B + 1]
        # a forward-only grid tower knows input_bn's statistics before the batch (the moving ones): gather and batch norm in one
        # launch, the same bits.  A training tower needs the batch statistics of r in between; a tower on selected
        # frames has a tenth of the rows and takes the two launches (7.20).
        fused_in = grid and not select and not self.training and not is_training and self.fused_input_pass
        if select:
            ops.frames_gather_packed_tab(x, num_frames, row_off, src, R, Rp, self.r, normalize=normalize)
        elif fused_in:
            bi.stats(None, R, False)
            ops.frames_gather_packed_bn(x, num_frames, row_off, self.every_n, R, Rp, bi.mean, bi.var, bi.gamma(), bi.beta(), self.r, self.r_bn,
                                        normalize=normalize)         # (rows R .. Rp of r_bn are zeros from the launch itself)
        elif grid:
            ops.frames_gather_packed(x, num_frames, row_off, self.every_n, R, Rp, self.r, normalize=normalize)
        else:
            R = self.R
            ops.sample_frames_gather(x, uniform, num_frames, self.r, self.idx, normalize=normalize)
        if not fused_in:
            bi.stats(self.r, R, is_training)
            ops.bn_apply(self.r, R, F, bi.mean, bi.var, bi.gamma(), bi.beta(), False, y_bf16=self.r_bn)
            if grid and Rp > R:
                self.r_bn[R:Rp].zero_()                      # (a longer earlier batch leaves stale rows there)
        ops.gemm_nt(self.r_bn, self.shadow_fwd[self.CW], R, K, F, self.act)
        bc.stats(self.act, R, is_training)
        ops.netvlad_softmax_fwd(self.act, R, K, bc.mean, bc.var, bc.gamma(), bc.beta(), self.a)
        if grid:
            ops.netvlad_aggregate_packed_fwd(self.a, self.r, row_off, B, self.T, K, F, R, plan.max_k, bi.mean, bi.var, bi.gamma(), bi.beta(),
                                             st.p(self.C2), self.Vv, self.asum)
        else:
            ops.netvlad_aggregate_fwd(self.a, self.r, B, S, K, F, bi.mean, bi.var, bi.gamma(), bi.beta(), st.p(self.C2), self.Vv, self.asum)
        ops.netvlad_normalize_fwd(self.Vv, B, K, F, self.n1, self.n2, self.Y_bf)
        ops.gemm_nt(self.Y_bf, self.shadow_fwd[self.HW], B, H, K * F, self.hid)
        self.bn_h.stats(self.hid, B, is_training)
        if not self.gating:
            ops.bn_apply(self.hid, B, H, self.bn_h.mean, self.bn_h.var, self.bn_h.gamma(), self.bn_h.beta(), True, y_f32=self.h6)
            head_in = self.h6
        else:
            bg = self.bn_g
            ops.bn_apply(self.hid, B, H, self.bn_h.mean, self.bn_h.var, self.bn_h.gamma(), self.bn_h.beta(), True, y_f32=self.h6, y_bf16=self.h6_bf)
            ops.gemm_nt(self.h6_bf, self.shadow_fwd[self.GW], B, H, H, self.gl)
            bg.stats(self.gl, B, is_training)
            if self.fused_gate:
                ops.bn_gate_fwd(self.gl, self.h6, B, H, bg.mean, bg.var, bg.gamma(), bg.beta(), self.gated)
            else:
                ops.bn_apply(self.gl, B, H, bg.mean, bg.var, bg.gamma(), bg.beta(), False, y_f32=self.gn)
                ops.nextvlad_gate_fwd(self.h6[:B], self.gn[:B], self.gated[:B])
            head_in = self.gated
        self._taped = self.training and is_training
        if B == self.cap:
            return self.moe.forward(head_in)
        return self.moe.forward(head_in[:B], rows=B)[:B]      # (a forward-only grid tower on fewer videos than it was allocated for)

    def grad_stages(self):
        moe = [MoeHead.GATES, MoeHead.EXPERTS, MoeHead.EBIAS]
        hidden = [self.HW, "hidden1_bn/beta", "hidden1_bn/gamma"]
        if self.gating:
            hidden += [self.GW, "gating_bn/beta", "gating_bn/gamma"]
        return moe, hidden, [k for k in self.names if k not in moe and k not in hidden]

    def _gate_backward(self, e, dstate):
        """The context gate's backward; e (+ dstate) is the gradient on `state`.  Leaves dh6_direct = e * g and dh6_via = dgl_bf . Wg^T,
        hidden1_bn's dy / dy2, and the gradients of gating_weights and gating_bn."""
        B, H, st, bg = self.B, self.Hd, self.store, self.bn_g
        stats = (bg.mean, bg.var, bg.gamma(), bg.beta())
        dgamma, dbeta = st.g("gating_bn/gamma"), st.g("gating_bn/beta")
        if self.fused_gate:
            ops.bn_gate_bwd_partial(self.gl, self.h6, e, dstate, B, H, *stats, bg.ws, self.dh6_direct)
            ops.bn_gate_bwd_finalize(self.gl, self.h6, e, dstate, B, bg.R_total, H, *stats, bg.ws, dgl_bf16=self.dgl_bf, dgamma=dgamma, dbeta=dbeta)
        else:
            ops.nextvlad_gate_bwd_add(self.h6, self.gn, e, dstate, self.dh6_direct, dgl=self.dgn)
            ops.bn_bwd_partial(self.gl, self.dgn, B, H, *stats, False, bg.ws)
            ops.bn_bwd_finalize(self.gl, self.dgn, B, bg.R_total, H, *stats, False, bg.ws, dx_bf16=self.dgl_bf, dgamma=dgamma, dbeta=dbeta)
        ops.gemm_tn(self.dgl_bf, self.h6_bf, H, H, self.Bk, st.g(self.GW))                # dWg^T [out][in] = dgl^T . h6
        ops.gemm_nt(self.dgl_bf, self.shadow_bwd[self.GW], B, H, H, self.dh6_via)

    def backward(self, dpred, on_moe_grads_ready=None, moe_weight_grads=True, on_stage=None, dstate=None):
        """dstate (None or [B, H] f32): a gradient on `state` itself, added to the MoE head's d(h6) in front of the relu6 mask of
        hidden1_bn's backward (BatchNorm.backward(dy2=...)); None keeps the plain launches."""
        assert self.training and self._taped, "backward needs a training-mode forward"
        B, F, S, K, H, R = self.B, self.F, self.S, self.Kc, self.Hd, self.R
        st, bi = self.store, self.bn_in
        if dstate is not None and tuple(dstate.shape) != (B, H):
            raise ValueError("dstate %s: the state of this tower is %s" % (tuple(dstate.shape), (B, H)))
        grid = self.frames == "grid"
        Rp = self.Rp if grid else R                          # row count of the TN product (grid: rows R .. Rp of its operands are zeros)
        dh6 = self.moe.backward(dpred, weight_grads=moe_weight_grads)
        if on_moe_grads_ready is not None:
            on_moe_grads_ready()
        if on_stage is not None:
            on_stage(0)
        if self.gating:
            self._gate_backward(dh6, dstate)
            self.bn_h.backward(self.hid, self.dh6_direct, B, True, dx_bf16=self.dhid_bf, dy2=self.dh6_via)
        elif dstate is None:
            self.bn_h.backward(self.hid, dh6, B, True, dx_bf16=self.dhid_bf)
        else:
            self.bn_h.backward(self.hid, dh6, B, True, dx_bf16=self.dhid_bf, dy2=dstate)
        ops.gemm_tn(self.dhid_bf, self.Y_bf, H, K * F, self.Bk, st.g(self.HW))          # dWh^T [H][K*F]
        if on_stage is not None:
            on_stage(1)
        ops.gemm_nt(self.dhid_bf, self.shadow_bwd[self.HW], B, K * F, H, self.dY)
        ops.netvlad_normalize_bwd(self.Vv, self.n1, self.n2, self.dY, B, K, F, self.dV)
        ops.netvlad_dcenters(self.asum, self.dV, B, K, F, st.g(self.C2))
        if grid:
            ops.netvlad_aggregate_packed_bwd(self.a, self.r, self.row_off[:B + 1], B, self.T, K, F, R, self.plan.max_k, bi.mean, bi.var, bi.gamma(),
                                             bi.beta(), st.p(self.C2), self.dV, self.da, self.dx, ws=self.agg_ws)
        else:
            ops.netvlad_aggregate_bwd(self.a, self.r, B, S, K, F, bi.mean, bi.var, bi.gamma(), bi.beta(), st.p(self.C2), self.dV, self.da, self.dx)
        ops.netvlad_softmax_bwd(self.a, self.da, R, K, self.dz)
        self.bn_cl.backward(self.act, self.dz, R, False, dx_bf16=self.dact_bf)
        if grid and Rp > R:
            self.dact_bf[R:Rp].zero_()
        ops.gemm_tn(self.dact_bf, self.r_bn, K, F, Rp, st.g(self.CW))                  # dWc^T [K][F]
        ops.gemm_nt(self.dact_bf, self.shadow_bwd[self.CW], R, F, K, self.dx, accumulate=True)   # + dact . Wc^T
        bi.backward(self.r, self.dx, R, False)
        if on_stage is not None:
            on_stage(2)

    def step_kwargs(self, global_step):
        """("random" frames are a function of the step too)"""
        return {"draw": global_step, "row0": 0} if self.sampling != "uniform" else {}

    @property
    def state(self):
        """The tower's representation, what its MoE head reads, [B, H] f32: h6 = relu6(hidden1_bn(hid)), or with the gate
        h6 * sigmoid(gating_bn(bf16(h6) . gating_weights))."""
        return self._live(self.gated if self.gating else self.h6)


def check_netvlad_gating(gating, world=1):
    """--netvlad_gating on more than one rank is refused; touches no device."""
    if gating and world > 1:
        raise ValueError("--netvlad_gating True refuses a process group of %d ranks: data parallelism is not built for the context gate "
                         "(gating_bn's statistics and gating_weights' gradient stay on one rank)" % world)


def check_netvlad_frames(frames, every_n, max_frames, model=None, world=1, precision="bf16", sampling="uniform"):
    """The combinations --netvlad_frames / --every_n / --student_sampling refuse, as ValueErrors that name the
    flags; touches no device."""
    if frames not in NetVladTower.FRAME_MODES:
        raise ValueError("--netvlad_frames %r: one of %s" % (frames, "|".join(NetVladTower.FRAME_MODES)))
    ops.check_student_sampling(sampling, "--student_sampling")
    if frames != "grid":
        if sampling != "uniform":
            raise ValueError("--student_sampling %s selects among the rows of --netvlad_frames grid; a %s tower draws its frames" % (sampling, frames))
        return
    if sampling != "uniform" and max_frames > ops.SELECT_MAX_T:
        raise ValueError("--student_sampling %s: --max_num_frames %d is refused, the source-frame tables hold at most %d frames per video"
                         % (sampling, max_frames, ops.SELECT_MAX_T))
    check_grid_frames(NetVladTower, frames, every_n, max_frames, model, world, precision)


def check_nextvlad_frames(frames, every_n, max_frames, model=None, world=1, precision="bf16"):
    """The combinations --nextvlad_frames / --every_n refuse, as ValueErrors that name the flags; touches no device."""
    if frames not in NeXtVladTower.FRAME_MODES:
        raise ValueError("--nextvlad_frames %r: one of %s" % (frames, "|".join(NeXtVladTower.FRAME_MODES)))
    if frames != "grid":
        return
    check_grid_frames(NeXtVladTower, frames, every_n, max_frames, model, world, precision)


class NeXtVladTower(VladTower):
    """NeXtVLAD aggregation tower (Lin, Xiao, Fan 2018) - an EXTENSION: the reference ships NeXtVLADModel as an empty stub
    (cs/frame_level_models.py:349-355), so there is no reference math; the binding definition is DESIGN.md 7.12, restated in
    float64 in tests/_nextvlad_ref.py: sample S frames -> expansion (.We + be, E = expansion * F) -> per group g of D = E / G
    columns: attention sigmoid(.Wa + ba) and softmax over K clusters of cluster_bn(.Wc) -> V[k] = sum_{s,g} a[s,g,k] (xe[s,g,:] -
    c2[k]) -> l2 per cluster -> vlad_bn -> .Wh -> hidden1_bn -> context gating (h * sigmoid(relu6(gating_bn(h.Wg1)).Wg2)) -> MoE.
    One stated deviation from the paper's code: relu6 where it has relu (the fused batch-norm tail knows relu6 only).  GEMM-shaped
    parts on the library's NT / TN kernels (bf16 operands, f32 accumulation), the f32 pieces in csrc/evc_nextvlad.hip.  V / U / Y
    and vlad_bn are kept cluster-major [K][D]; the TF order d*K + k of vlad_bn/* and of hidden1_weights' rows is restored in
    state_dict().

    frames="grid" (DESIGN.md 7.13): instead of S drawn frames, video b contributes the frames j * every_n < min(n_b, T) - every real
    frame at every_n = 1, the fewer-frames student's grid above - as a ragged list of rows packed back to back (ops.GridPlan);
    padding frames are never computed.  Same weights and checkpoint names: a tower of either mode loads the other's checkpoint.

    Distillation: `state` is the gated hidden vector `out` [B, H], the representation L_REP is taken on, and
    backward(dpred, dstate=...) adds a gradient on it to the MoE head's.  A forward-only grid tower (training=False: the frozen
    teacher) keeps no gradient store or moments and aggregates on the f32 matrix cores (evc_nextvlad_aggregate_packed_fwd_mfma, the
    bits of the entry the training towers call).

    Dropout: dropout = the DROP rate in [0, 1) on the hidden layer's operand in training-mode forwards of a training
    tower, Yd = vlad_bn(U) * m / (1 - rate).  m is a stateless function of (dropout_seed, rank, dropout_step, element) evaluated inside
    the kernel that writes Y_bf (ops.nextvlad_dropout_fwd, in place of that bn_apply) and again in backward (ops.nextvlad_dropout_bwd on
    dY); no mask is stored.  rank is the data-parallel rank of the group the step reduces over - process_group, or the default group
    when none is given, as train.main builds the tower - so ranks drop different elements.  At rate 0, with is_training=False or on
    a forward-only tower the launches are the ones without the feature."""

    FAMILY, MODEL, FLAG, NOT_A_CHECKPOINT = "NeXtVLAD", "NeXtVLADModel", "--nextvlad", "not a NeXtVLADModel checkpoint of that tower"

    EW, EB, AW, AB = "expansion_weights", "expansion_biases", "attention_weights", "attention_biases"
    CW, C2, HW, G1, G2 = "cluster_weights", "cluster_weights2", "hidden1_weights", "gating_weights_1", "gating_weights_2"
    BNS = ("cluster_bn", "vlad_bn", "hidden1_bn", "gating_bn")
    l2_names = (MoeHead.GATES, MoeHead.EXPERTS)
    # all four batch-norms go through BatchNorm.backward: their gamma/beta gradients are global (all-reduced f64 sums)
    global_grad_names = tuple("%s/%s" % (s_, v) for s_ in BNS for v in ("beta", "gamma"))
    AP = 64                            # rows of the attention operand image / columns of the attention logits (one GEMM tile)

    def __init__(self, batch_size, max_frames=300, feature_size=1152, vocab_size=4716, iterations=30, cluster_size=64,
                 hidden_size=1024, groups=8, expansion=2, gating_reduction=8, num_mixtures=2, device="cuda:0", training=True,
                 scope="model", seed=0, process_group=None, frames="sampled", every_n=1, dropout=0.0, dropout_seed=0):
        world = 1
        if process_group is not None and torch.distributed.is_available() and torch.distributed.is_initialized():
            world = torch.distributed.get_world_size(process_group)
        check_nextvlad_frames(frames, every_n, max_frames, world=world)          # (before the device is touched)
        # The Philox key's rank: that of the group the step's reductions run over.  BatchNorm and GradReducer fall back to the DEFAULT
        # group when process_group is None (train.main builds the tower that way under a launcher), so the rank does too.
        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank(process_group)
        self.dropout_seed, self.rank = int(dropout_seed), int(rank)
        self.set_dropout(dropout)
        self._drop = None                                                        # (T, scale, step) of the last forward that dropped
        self.frames, self.every_n = frames, int(every_n)
        self.device, self.training, self.scope, self.pg = torch.device(device), training, scope, process_group
        self.T, self.F, self.V, self.S = max_frames, feature_size, vocab_size, iterations
        self.Kc, self.Hd, self.Mx, self.G = cluster_size, hidden_size, num_mixtures, groups
        if groups < 1 or expansion < 1 or gating_reduction < 1 or cluster_size < 1:
            raise ValueError("groups=%d, expansion=%d, gating_reduction=%d, cluster_size=%d must all be >= 1"
                             % (groups, expansion, gating_reduction, cluster_size))
        F, K, H, G = feature_size, cluster_size, hidden_size, groups
        E = self.E = expansion * F
        if E % G:
            raise ValueError("expanded width %d (expansion %d x %d features) is not a multiple of groups=%d" % (E, expansion, F, G))
        D = self.D = E // G
        if hidden_size % gating_reduction:
            raise ValueError("hidden_size=%d is not a multiple of gating_reduction=%d" % (hidden_size, gating_reduction))
        Hg = self.Hg = hidden_size // gating_reduction
        for what, n in (("feature_size", F), ("expanded width", E), ("groups x cluster_size", G * K), ("cluster_size x group width", K * D),
                        ("hidden_size", H), ("hidden_size / gating_reduction", Hg)):
            if n % 64:
                raise ValueError("%s = %d must be a multiple of 64 for the MFMA GEMM tiles" % (what, n))
        if D % 4:
            raise ValueError("group width %d (expanded width %d / groups %d) must be a multiple of 4 for the aggregation kernels" % (D, E, G))
        if G > self.AP:
            raise ValueError("groups=%d: the attention product holds at most %d groups" % (G, self.AP))
        if K > 1024:
            raise ValueError("cluster_size=%d: the assignment kernel holds at most 1024 clusters" % K)
        if frames == "sampled" and iterations > 64:                  # (grid mode does not read iterations)
            raise ValueError("iterations=%d: the aggregation kernels hold at most 64 sampled frames per video" % iterations)
        if frames == "sampled" and iterations * G > 1024:
            raise ValueError("iterations x groups = %d: the aggregation kernels hold at most 1024 (frame, group) pairs per video" % (iterations * G))
        shapes = self.variable_shapes(F, vocab_size, K, H, G, expansion, gating_reduction, num_mixtures)
        self.buffers = OrderedDict()
        self._setup_store(shapes)
        # the attention product has N = G columns, below the GEMM tiles' width: its forward operand is the first G rows of a
        # zero-padded [AP][E] image (every writer of shadow_fwd - casts, the fused Adam pass - writes through the view)
        self.att_img = torch.zeros((self.AP, E), dtype=BF16, device=self.device)
        self.shadow_fwd[self.AW] = self.att_img[:G]
        self.bn_cl = BatchNorm(self, "cluster_bn", G * K)
        self.bn_v = BatchNorm(self, "vlad_bn", K * D)
        self.bn_h = BatchNorm(self, "hidden1_bn", H)
        self.bn_g = BatchNorm(self, "gating_bn", Hg)
        self.moe = MoeHead(self, H, vocab_size, num_mixtures)
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed)
        for k, shp in self.store.shapes.items():
            p = self.store.p(k)
            if k in (self.EW, self.AW, self.CW, self.G1, self.G2):
                p.copy_(torch.randn(shp, generator=gen, dtype=F32) / math.sqrt(shp[1]))
            elif k == self.C2:
                p.copy_(torch.randn(shp, generator=gen, dtype=F32) / math.sqrt(D))
            elif k == self.HW:
                p.copy_(torch.randn(shp, generator=gen, dtype=F32) / math.sqrt(K))
            elif len(shp) == 2:
                lim = math.sqrt(6.0 / (shp[0] + shp[1]))
                p.copy_((torch.rand(shp, generator=gen, dtype=F32) * 2 - 1) * lim)
            elif k.endswith("/gamma"):
                p.fill_(1.0)
        self.refresh_shadows()
        if not training and frames == "grid":
            self.store.drop_training_state()                         # forward only: the masters alone, as the frozen H-LSTM teacher
        self._alloc(batch_size)

    def set_dropout(self, rate):
        """The DROP rate in [0, 1) (a ValueError names any other value) and, from it, the constants of the two dropout entries: the
        threshold T = floor(keep * 2^32) and the scale float32(1 / keep).  0: the feature makes no launch."""
        self.dropout = ops.check_dropout_rate(rate)
        self._drop_T, self._drop_scale = ops.dropout_threshold(1.0 - self.dropout) if self.dropout > 0.0 else (0, 1.0)

    @classmethod
    def variable_shapes(cls, feature_size, vocab_size, cluster_size, hidden_size, groups, expansion, gating_reduction, num_mixtures):
        """The trainable variables and their INTERNAL shapes, in store order, from the size flags alone (no device)."""
        F, K, H, G = feature_size, cluster_size, hidden_size, groups
        E = expansion * F
        D, Hg = E // G, hidden_size // gating_reduction
        shapes = OrderedDict()
        shapes[cls.EW] = (E, F)                                      # every 2-D weight is stored transposed [out][in]
        shapes[cls.EB] = (E,)
        shapes[cls.AW] = (G, E)
        shapes[cls.AB] = (G,)
        shapes[cls.CW] = (G * K, E)
        shapes.update(BatchNorm.shapes("cluster_bn", G * K))
        shapes[cls.C2] = (K, D)                                      # centres [K][D] (tf: [D, K])
        shapes.update(BatchNorm.shapes("vlad_bn", K * D))            # cluster-major k*D + d
        shapes[cls.HW] = (H, K * D)                                  # columns cluster-major
        shapes.update(BatchNorm.shapes("hidden1_bn", H))
        shapes[cls.G1] = (Hg, H)
        shapes.update(BatchNorm.shapes("gating_bn", Hg))
        shapes[cls.G2] = (H, Hg)
        shapes.update(MoeHead.shapes(H, vocab_size, num_mixtures))
        return shapes

    # TF order d*K + k  <->  internal cluster-major k*D + d: the rows of hidden1_weights [K*D, H] and every vlad_bn vector
    def _tf_keys(self, prefix):
        return ["%s/vlad_bn/%s" % (prefix, v) for v in ("beta", "gamma", "moving_mean", "moving_variance")]

    def state_dict(self):
        out = super().state_dict()
        K, D, H = self.Kc, self.D, self.Hd
        key = "%s/%s" % (self.scope, self.HW)
        out[key] = out[key].view(K, D, H).permute(1, 0, 2).reshape(D * K, H).contiguous()
        for key in self._tf_keys(self.scope):
            out[key] = out[key].view(K, D).t().reshape(D * K).contiguous()
        return out

    def load_state_dict(self, sd, prefix=None):
        prefix = self.scope if prefix is None else prefix
        K, D, H = self.Kc, self.D, self.Hd
        key = "%s/%s" % (prefix, self.HW)
        if key not in sd:
            raise KeyError("NeXtVladTower.load_state_dict: %r is not in the checkpoint (scope prefix %r; it holds e.g. %s)"
                           % (key, prefix, sorted(sd)[:3]))
        sd = dict(sd)
        sd[key] = sd[key].view(D, K, H).permute(1, 0, 2).reshape(K * D, H).contiguous()
        for key in self._tf_keys(prefix):
            if key in sd:
                sd[key] = sd[key].view(D, K).t().reshape(K * D).contiguous()
        super().load_state_dict(sd, prefix)

    def _alloc(self, B):
        dev, F, S, K, H, G, E, D, Hg, AP = self.device, self.F, self.S, self.Kc, self.Hd, self.G, self.E, self.D, self.Hg, self.AP
        grid = self.frames == "grid"
        # (grid: the bf16 operands of the TN products start as zeros; their rows R .. Rp are zeroed again at every step.  A forward-only
        # tower can serve a subset of the batch's videos, forward(sel=...))
        R = self._alloc_rows(B, with_sel=not self.training)
        self.r = torch.empty((R, F), dtype=F32, device=dev)
        if not grid:
            self.idx = torch.empty((B, S), dtype=torch.int32, device=dev)
        self.r_bf = torch.zeros((R, F), dtype=BF16, device=dev) if grid else torch.empty((R, F), dtype=BF16, device=dev)
        self.xe = torch.empty((R, E), dtype=F32, device=dev)
        self.xe_bf = torch.zeros((R, E), dtype=BF16, device=dev) if grid else torch.empty((R, E), dtype=BF16, device=dev)
        self.attl = torch.empty((R, AP), dtype=F32, device=dev)      # attention logits, biases included (columns >= G: zeros)
        self.cbias = torch.empty((G * K,), dtype=F32, device=dev)    # be . Wc: what the expansion bias adds to every cluster logit
        self.abias = torch.empty((AP,), dtype=F32, device=dev)       # be . Wa + ba (entries >= G: zeros)
        self.act = torch.empty((R, G * K), dtype=F32, device=dev)
        self.a = torch.empty((R, G * K), dtype=F32, device=dev)
        self.asum = torch.empty((B, K), dtype=F32, device=dev)
        self.Vv = torch.empty((B, K, D), dtype=F32, device=dev)
        self.nrm = torch.empty((B, K), dtype=F32, device=dev)
        self.U = torch.empty((B, K * D), dtype=F32, device=dev)
        self.Y_bf = torch.zeros((self.Bk, K * D), dtype=BF16, device=dev)
        self.hid = torch.empty((B, H), dtype=F32, device=dev)
        self.h = torch.empty((B, H), dtype=F32, device=dev)
        self.h_bf = torch.zeros((self.Bk, H), dtype=BF16, device=dev)
        self.g1pre = torch.empty((B, Hg), dtype=F32, device=dev)
        self.g1_bf = torch.zeros((self.Bk, Hg), dtype=BF16, device=dev)
        self.gl = torch.empty((B, H), dtype=F32, device=dev)
        self.out = torch.empty((B, H), dtype=F32, device=dev)
        self.moe.alloc(B, self.training)
        if self.training:
            self.dh = torch.empty((B, H), dtype=F32, device=dev)
            self.dgl_bf = torch.zeros((self.Bk, H), dtype=BF16, device=dev)
            self.dg1 = torch.empty((B, Hg), dtype=F32, device=dev)
            self.dg1pre_bf = torch.zeros((self.Bk, Hg), dtype=BF16, device=dev)
            self.dhid_bf = torch.zeros((self.Bk, H), dtype=BF16, device=dev)
            self.dY = torch.empty((B, K * D), dtype=F32, device=dev)
            self.dU = torch.empty((B, K * D), dtype=F32, device=dev)
            self.dV = torch.empty((B, K, D), dtype=F32, device=dev)
            self.agg_ws = torch.empty(ops.nextvlad_aggregate_bwd_ws(B, K, D), dtype=F32, device=dev)
            self.da = torch.empty((R, G * K), dtype=F32, device=dev)
            self.dz = torch.empty((R, G * K), dtype=F32, device=dev)
            self.dact_bf = torch.zeros((R, G * K), dtype=BF16, device=dev) if grid else torch.empty((R, G * K), dtype=BF16, device=dev)
            self.datt = torch.empty((R, G), dtype=F32, device=dev)
            self.datt_bf = torch.zeros((R, AP), dtype=BF16, device=dev)     # columns >= G stay zero
            self.dxe = torch.empty((R, E), dtype=F32, device=dev)
            self.dxe_bf = torch.zeros((R, E), dtype=BF16, device=dev) if grid else torch.empty((R, E), dtype=BF16, device=dev)
            self.colsum_ws = torch.empty(32 * E, dtype=F32, device=dev)    # partial rows of the two bias-gradient column sums
            self.dWa_pad = torch.empty((AP, E), dtype=F32, device=dev)      # the attention weight gradient on a whole tile of rows

    def forward(self, x, num_frames, uniform=None, normalize=True, is_training=True, num_frames_host=None, sel=None, dropout_step=0):
        """x [B,T,F] float32 or uint8 raw frames; uniform [B,S] f32 in [0,1): the frame-sampling draw (sampled mode; not read
        in grid mode, which takes num_frames_host, the frame counts on the host, instead).
        A forward-only grid tower keeps the buffers it allocated: a batch of fewer videos uses their first rows.  sel (such a tower
        only): a strictly ascending host sequence of video numbers - the tower runs on those b' videos of the
        unchanged batch alone, and pred / state hold b' rows, row j for video sel[j].
        dropout_step: the graph's global_step (a host integer), the counter of this forward's dropout mask; backward() regenerates the
        mask from the step this forward used.  Not read at rate 0, with is_training=False or on a forward-only tower."""
        B = x.shape[0]
        serving = self.frames == "grid" and not self.training
        if sel is not None:
            if not serving:
                raise ValueError("forward(sel=...) is built for forward-only grid towers (training=False, frames='grid')")
            sel = ops.check_row_selection(sel, B)                    # (on the host, before any launch)
            B = int(sel.shape[0])
        self._fit_batch(B)
        if self.precision != "bf16":
            raise NotImplementedError("NeXtVladTower has no split-bf16 mode")
        grid = self.frames == "grid"
        F, S, K, H, G, E, D, Hg, AP = self.F, self.S, self.Kc, self.Hd, self.G, self.E, self.D, self.Hg, self.AP
        st, bc, bv, bh, bg = self.store, self.bn_cl, self.bn_v, self.bn_h, self.bn_g
        if grid:
            if x.shape[1] != self.T:
                raise ValueError("the batch holds %d frames per video, the tower was built for max_frames=%d" % (x.shape[1], self.T))
            plan = self._plan_grid_rows(num_frames, num_frames_host, sel)
            R, Rp = plan.R, plan.Rp
            row_off = self.row_off[:B + 1]
            if sel is None:
                ops.frames_gather_packed(x, num_frames, row_off, self.every_n, R, Rp, self.r, self.r_bf, normalize=normalize)
            else:                                                # (the forward reads the bf16 rows alone)
                ops.frames_gather_packed_sel(x, num_frames, row_off, self.sel[:B], self.every_n, R, Rp, None, self.r_bf, normalize=normalize)
        else:
            R = self.R
            ops.sample_frames_gather(x, uniform, num_frames, self.r, self.idx, normalize=normalize)
            ops.cast_bf16(self.r, self.r_bf)
        ops.gemm_nt(self.r_bf, self.shadow_fwd[self.EW], R, E, F, self.xe, bias=st.p(self.EB))
        # The bf16 operand of the two logit products is xe - be: the bias is the same in every row, so rounding it into the operand
        # would spend bf16's 8 bits on a constant whose whole effect on a logit is the per-column constant be.W - that goes into the
        # products as their f32 bias instead (and cluster_bn removes it again in training).  xe itself stays f32 for the aggregation.
        ops.nextvlad_center_cast(self.xe, R, E, st.p(self.EB), self.xe_bf)
        if grid and Rp > R:
            self.xe_bf[R:Rp].zero_()                         # (a longer earlier batch leaves stale rows there)
        ops.nextvlad_bias_logits(st.p(self.EB), st.p(self.CW), G * K, E, self.cbias)
        ops.nextvlad_bias_logits(st.p(self.EB), st.p(self.AW), G, E, self.abias, add=st.p(self.AB))
        ops.gemm_nt(self.xe_bf, self.shadow_fwd[self.CW], R, G * K, E, self.act, bias=self.cbias)
        ops.gemm_nt(self.xe_bf, self.att_img, R, AP, E, self.attl, bias=self.abias)
        bc.stats(self.act, R, is_training)
        ops.nextvlad_assign_fwd(self.act, R, G, K, bc.mean, bc.var, bc.gamma(), bc.beta(), self.attl, self.a)
        if grid:
            agg = ops.nextvlad_aggregate_packed_fwd if self.training else ops.nextvlad_aggregate_packed_fwd_mfma      # (the same bits)
            agg(self.a, self.xe, row_off, B, self.T, G, K, D, R, plan.max_k, st.p(self.C2), self.Vv, self.asum)
        else:
            ops.nextvlad_aggregate_fwd(self.a, self.xe, B, S, G, K, D, st.p(self.C2), self.Vv, self.asum)
        ops.nextvlad_normalize_fwd(self.Vv, B, K, D, self.U, self.nrm)
        bv.stats(self.U, B, is_training)
        self._drop = None
        if self.dropout > 0.0 and self.training and is_training:
            self._drop = (self._drop_T, self._drop_scale, int(dropout_step))
            ops.nextvlad_dropout_fwd(self.U, B, K * D, bv.mean, bv.var, bv.gamma(), bv.beta(), *self._drop[:2], self.dropout_seed, self.rank,
                                     self._drop[2], self.Y_bf)
        else:
            ops.bn_apply(self.U, B, K * D, bv.mean, bv.var, bv.gamma(), bv.beta(), False, y_bf16=self.Y_bf)
        ops.gemm_nt(self.Y_bf, self.shadow_fwd[self.HW], B, H, K * D, self.hid)
        bh.stats(self.hid, B, is_training)
        ops.bn_apply(self.hid, B, H, bh.mean, bh.var, bh.gamma(), bh.beta(), False, y_f32=self.h, y_bf16=self.h_bf)
        ops.gemm_nt(self.h_bf, self.shadow_fwd[self.G1], B, Hg, H, self.g1pre)
        bg.stats(self.g1pre, B, is_training)
        ops.bn_apply(self.g1pre, B, Hg, bg.mean, bg.var, bg.gamma(), bg.beta(), True, y_bf16=self.g1_bf)
        ops.gemm_nt(self.g1_bf, self.shadow_fwd[self.G2], B, H, Hg, self.gl)
        ops.nextvlad_gate_fwd(self.h[:B], self.gl[:B], self.out[:B])
        self._taped = self.training and is_training
        if B == self.cap:
            return self.moe.forward(self.out)
        return self.moe.forward(self.out[:B], rows=B)[:B]         # (a forward-only grid tower on fewer videos than it was allocated for)

    def grad_stages(self):
        moe = [MoeHead.GATES, MoeHead.EXPERTS, MoeHead.EBIAS]
        hidden = [self.G2, "gating_bn/beta", "gating_bn/gamma", self.G1, "hidden1_bn/beta", "hidden1_bn/gamma", self.HW]
        return moe, hidden, [k for k in self.names if k not in moe and k not in hidden]

    def backward(self, dpred, on_moe_grads_ready=None, moe_weight_grads=True, on_stage=None, dstate=None):
        """dstate (None or [B, H] f32): a gradient on `state` itself, added to the MoE head's d(out) in the gate backward."""
        assert self.training and self._taped, "backward needs a training-mode forward"
        B, F, S, K, H, R, G, E, D, Hg, AP = self.B, self.F, self.S, self.Kc, self.Hd, self.R, self.G, self.E, self.D, self.Hg, self.AP
        st, bc = self.store, self.bn_cl
        grid = self.frames == "grid"
        Rp = self.Rp if grid else R                          # row count of the TN products (grid: rows R .. Rp of their operands are zeros)
        dout = self.moe.backward(dpred, weight_grads=moe_weight_grads)
        if on_moe_grads_ready is not None:
            on_moe_grads_ready()
        if on_stage is not None:
            on_stage(0)
        # context gating
        if dstate is None:
            ops.nextvlad_gate_bwd(self.h, self.gl, dout, self.dh, dgl_bf16=self.dgl_bf)
        else:
            if dstate.shape != self.out.shape:
                raise ValueError("dstate %s: the state of this tower is %s" % (tuple(dstate.shape), tuple(self.out.shape)))
            ops.nextvlad_gate_bwd_add(self.h, self.gl, dout, dstate, self.dh, dgl_bf16=self.dgl_bf)
        ops.gemm_tn(self.dgl_bf, self.g1_bf, H, Hg, self.Bk, st.g(self.G2))              # dWg2^T [H][Hg]
        ops.gemm_nt(self.dgl_bf, self.shadow_bwd[self.G2], B, Hg, H, self.dg1)
        self.bn_g.backward(self.g1pre, self.dg1, B, True, dx_bf16=self.dg1pre_bf)
        ops.gemm_tn(self.dg1pre_bf, self.h_bf, Hg, H, self.Bk, st.g(self.G1))           # dWg1^T [Hg][H]
        ops.gemm_nt(self.dg1pre_bf, self.shadow_bwd[self.G1], B, H, Hg, self.dh, accumulate=True)
        # hidden layer
        self.bn_h.backward(self.hid, self.dh, B, False, dx_bf16=self.dhid_bf)
        ops.gemm_tn(self.dhid_bf, self.Y_bf, H, K * D, self.Bk, st.g(self.HW))          # dWh^T [H][K*D]
        if on_stage is not None:
            on_stage(1)
        ops.gemm_nt(self.dhid_bf, self.shadow_bwd[self.HW], B, K * D, H, self.dY)
        if self._drop is not None:                           # dY = dYd * m / keep: the mask of this forward, regenerated
            ops.nextvlad_dropout_bwd(self.dY, B, K * D, self._drop[0], self._drop[1], self.dropout_seed, self.rank, self._drop[2])
        self.bn_v.backward(self.U, self.dY, B, False, dx_f32=self.dU)
        ops.nextvlad_normalize_bwd(self.Vv, self.nrm, self.dU, B, K, D, self.dV)
        ops.netvlad_dcenters(self.asum, self.dV, B, K, D, st.g(self.C2))                 # the same sum as NetVLAD's centres
        if grid:
            ops.nextvlad_aggregate_packed_bwd(self.a, self.xe, self.row_off, B, self.T, G, K, D, R, self.plan.max_k, st.p(self.C2), self.dV,
                                              self.da, self.dxe, ws=self.agg_ws)
        else:
            ops.nextvlad_aggregate_bwd(self.a, self.xe, B, S, G, K, D, st.p(self.C2), self.dV, self.da, self.dxe, ws=self.agg_ws)
        ops.nextvlad_assign_bwd(self.act, R, G, K, bc.mean, bc.var, bc.gamma(), bc.beta(), self.attl, self.da, self.dz, self.datt,
                                datt_logit_bf16=self.datt_bf)
        bc.backward(self.act, self.dz, R, False, dx_bf16=self.dact_bf)
        if grid and Rp > R:
            self.dact_bf[R:Rp].zero_()
            self.datt_bf[R:Rp].zero_()
        # xe_bf is the CENTRED operand xe - be.  dWc = dact^T . xe = dact^T . (xe - be) + colsum(dact) (x) be, and the column sums of a
        # training-mode batch-norm's input gradient are zero: the product against the centred operand is the whole gradient.
        ops.gemm_tn(self.dact_bf, self.xe_bf, G * K, E, Rp, st.g(self.CW))               # dWc^T [G*K][E]
        ops.gemm_nt(self.dact_bf, self.shadow_bwd[self.CW], R, E, G * K, self.dxe, accumulate=True)      # + dact . Wc^T
        # the attention logits have no batch-norm behind them: dWa = datt^T . (xe - be) + dba (x) be, dba = colsum(datt)
        ops.nextvlad_colsum(self.datt, R, G, st.g(self.AB), ws=self.colsum_ws)
        ops.gemm_tn(self.datt_bf, self.xe_bf, AP, E, Rp, self.dWa_pad)                   # on a whole tile of rows, rows >= G are zero
        ops.nextvlad_wgrad_uncenter(self.dWa_pad, st.g(self.AB), st.p(self.EB), G, E, st.g(self.AW))
        ops.gemm_nt(self.datt_bf, self.shadow_bwd[self.AW], R, E, AP, self.dxe, accumulate=True)         # + datt . Wa^T
        ops.nextvlad_colsum(self.dxe, R, E, st.g(self.EB), ws=self.colsum_ws)
        ops.cast_bf16(self.dxe[:R], self.dxe_bf[:R])
        if grid and Rp > R:
            self.dxe_bf[R:Rp].zero_()
        ops.gemm_tn(self.dxe_bf, self.r_bf, E, F, Rp, st.g(self.EW))                     # dWe^T [E][F]
        if on_stage is not None:
            on_stage(2)

    def step_kwargs(self, global_step):
        """(the dropout mask is a function of the step: a restored run draws the same masks)"""
        return {"dropout_step": global_step}

    state = property(lambda self: self._live(self.out))


class LogisticTower(TowerBase):
    """FrameLevelLogisticModel: sigmoid(mean_frames(x) . W + b), with the
    reference's quirk that the sum runs over all (zero-padded) frames and is
    divided by the true frame count (cs/frame_level_models.py:72-78)."""

    W, Bn = "fully_connected/weights", "fully_connected/biases"
    l2_names = ("fully_connected/weights",)                      # weights_regularizer=slim.l2_regularizer(1e-8)

    def __init__(self, batch_size, max_frames=300, feature_size=1152, vocab_size=4716, device="cuda:0",
                 training=True, scope="model", seed=0):
        self.device, self.training, self.scope = torch.device(device), training, scope
        self.T, self.F, self.V = max_frames, feature_size, vocab_size
        if feature_size % 64:
            raise ValueError("feature_size must be a multiple of 64 for the MFMA GEMM tiles")
        shapes = OrderedDict([(self.W, (vocab_size, feature_size)), (self.Bn, (vocab_size,))])
        self._setup_store(shapes)
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed)
        lim = math.sqrt(6.0 / (vocab_size + feature_size))
        self.store.p(self.W).copy_((torch.rand((vocab_size, feature_size), generator=gen, dtype=F32) * 2 - 1) * lim)
        self.refresh_shadows()
        self._alloc(batch_size)

    def _alloc(self, B):
        dev, F, V = self.device, self.F, self.V
        self.B = B
        self.avg = torch.empty((B, F), dtype=F32, device=dev)
        self.avg_bf = torch.empty((B, F), dtype=BF16, device=dev)
        self.pred = torch.empty((B, V), dtype=F32, device=dev)
        if self.training:
            self.Bp = ops.round_up(B, 64)
            self.dz = torch.empty((B, V), dtype=BF16, device=dev)
            self.dzT = torch.empty((V, self.Bp), dtype=BF16, device=dev)
            self.avgT = torch.empty((F, self.Bp), dtype=BF16, device=dev)

    def forward(self, x, num_frames, normalize=True):
        B = x.shape[0]
        if B != self.B:
            self._alloc(B)
        ops.meanpool(x, num_frames, self.avg, self.avg_bf, normalize=normalize)
        if self.precision != "bf16":
            if not hasattr(self, "avg_lo") or self.avg_lo.shape != self.avg_bf.shape:
                self.avg_lo = torch.empty_like(self.avg_bf)
            ops.cast_bf16_split(self.avg, self.avg_bf, self.avg_lo)
            ops.gemm_nt_split(self.avg_bf, self.avg_lo, self.shadow_fwd[self.W], self.shadow_lo[self.W], B, self.V, self.F,
                              self.pred, bias=self.store.p(self.Bn))
        else:
            ops.gemm_nt(self.avg_bf, self.shadow_fwd[self.W], B, self.V, self.F, self.pred, bias=self.store.p(self.Bn))
        ops.sigmoid_(self.pred)
        return self.pred

    def grad_stages(self):
        return ([self.W, self.Bn],)

    def backward(self, dpred, on_moe_grads_ready=None, moe_weight_grads=True, on_stage=None):
        B, V, F = self.B, self.V, self.F
        ops.sigmoid_bwd(self.pred, dpred, self.dz)
        ops.transpose_to_bf16(self.dz, B, V, self.dzT, self.Bp)
        ops.transpose_to_bf16(self.avg_bf, B, F, self.avgT, self.Bp)
        ops.gemm_nt(self.dzT, self.avgT, V, F, self.Bp, self.store.g(self.W))
        ops.rowsum_bf16(self.dzT, V, self.Bp, self.store.g(self.Bn))
        if on_moe_grads_ready is not None:
            on_moe_grads_ready()
        if on_stage is not None:
            on_stage(0)
