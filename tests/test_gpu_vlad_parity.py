"""The VLAD kernels (csrc/evc_nextvlad.hip, csrc/evc_netvlad.hip) through their ops wrappers: every element of everything an entry stores
against the float64 reference of tests/_vlad_ref.py, within the bound derived there, at shapes that reach the second column tile, the
second row tile and the later contraction passes of nx_product_kernel, registers i >= 1 of the softmaxes, the second s0 chunk and
F4 >= 256 of the NetVLAD aggregation, the clamps, the empty last row range of the two-pass colsum and the grid-stride tails.  Every output
buffer is prefilled with NaN and is larger than the output (a guard row behind it; guard columns where the entry takes a row stride);
_vlad_ref.judge asserts that every owned element is finite and within its bound (none exempt) and that the guards keep their NaN.  Every
entry runs twice and must repeat bit for bit.  Bit-for-bit identities: the mfma packed forward == the vector one, packed == fixed-length
on equal lengths, every bf16 copy == bf16 of its f32 twin, gate_bwd_add(dout2=None) == gate_bwd, videos without frames give exact zeros.
pytest -m gpu; every check prints `ratio gpu <entry> <case> <output> <worst got/bound> at <index>` (pytest -s shows the lines).

What fails where, were a path disabled (tests/test_cpu_vlad_ref.py plants these in the emulations; (B,S,G,K,D) names a fixed-length case):
    the l0 > 0 passes   MODE 0: (3,30,8,64,288), P = 240: V[0,0,0] lacks the pairs 64..239;  MODE 1: (2,7,3,65,68): dxe[0,0] lacks k = 64;
                        MODE 2: the same case, D = 68: da[0,0] lacks d = 64..67
    ntile > 0           (2,7,3,65,68): the one live lane of column tile 1 owns V[0,0,64..67], dxe[0,64..67] and da[0,64] (Kp = 68)
    mtile > 0           MODE 0: (1,64,16,130,260), MT = 64: V[0,64,0] (and its sa[]);  MODE 1 / 2: (3,30,8,64,288), MT = 128: dxe[128,0], da[128,0]
    packed offsets      G=3 K=65 D=68 ks=0,22,1,43,0: V[2,0,0] is the one frame of video 2; dxe / da rows 66..68 are its rows
    registers i >= 1    assign / softmax K = 65: a[r,g,64] is register 1 of lane 0; K >= 65, row 2: the maximum (+50) sits in the last cluster
                        over -50 elsewhere, and exp(100) of a maximum over register 0 alone is not finite
    second s0 chunk     NetVLAD (2,17,5,260): dx[0,16,:] is the one frame of the second chunk (NaN if never stored)
    F4 >= 256           NetVLAD (2,64,13,1028): V[0,0,1024..1027] is thread 0's second float4
    the clamps          nextvlad_normalize (2,7,12): U[0,0,:] = 0 / 0 without it;  netvlad_normalize: Y[0,1,:] and the all-zero last video
    grid-stride tails   gate n = 8192 * 256 + 259: out[8192 * 256];  center_cast (8161,1028): the last 225 float4s;  wgrad_uncenter (2049,1025)
                        and dcenters (1,2049,4100): the last 3073 items - a NaN left where a value is owed

Measured on an MI355X: profiles/vlad_parity_ratios.txt.
"""
import numpy as np
import pytest
import torch

import _vlad_ref as vr
from _vlad_ref import F32
from efficientvideoclassification_youtube8m_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(autouse=True)
def _stop_on_a_gpu_error():
    """A GPU fault ends the session: nothing more is started on a device that a kernel of this file has just faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:   # a sticky HIP error
        pytest.exit("GPU error after a VLAD parity test, stopping: %s" % e, returncode=3)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def host(t):
    """numpy of a device tensor; bf16 as bit patterns (uint16)."""
    if t.dtype == BF16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def twice(run):
    """run() -> dict of freshly allocated device outputs; a second run must give the same bits.  Returns the first as numpy."""
    a, b = run(), run()
    torch.cuda.synchronize()
    for k in a:
        assert same_bits(a[k], b[k]), "%s did not repeat bit for bit" % k
    return {k: host(v) for k, v in a.items()}


class Report:
    def __init__(self, entry):
        self.entry, self.bad, self.n = entry, [], 0

    def add(self, case, q):
        for out, arr in q.items():
            r, at = vr.worst(arr)
            line = "ratio gpu %s %s %s %.4f at %s" % (self.entry, case, out, r, at)
            print(line)
            self.n += 1
            if not r <= 1.0:
                self.bad.append(line)

    def done(self):
        assert self.n > 0 and not self.bad, "\n".join(self.bad)


# ---------------------------------------------------------------------------- NeXtVLAD products
def _agg_inputs(c):
    return dev(c.a), dev(c.xe), dev(c.c2), dev(c.dV)


def _agg_fixed(c, a, xe, c2, dV):
    B, S, G, K, D, Pt = c.B, c.S, c.G, c.K, c.D, c.B * c.S * c.G

    def run():
        V, asum, dxe, da = nan(B + 1, K, D), nan(B + 1, K), nan(Pt + 1, D), nan(Pt + 1, K)
        ops.nextvlad_aggregate_fwd(a, xe, B, S, G, K, D, c2, V, asum)
        ops.nextvlad_aggregate_bwd(a, xe, B, S, G, K, D, c2, dV, da, dxe)
        return dict(V=V, asum=asum, dxe=dxe, da=da)
    return run


def _agg_packed(c, a, xe, c2, dV, fwd):
    B, G, K, D, Pt = c.B, c.G, c.K, c.D, c.R * c.G
    off = dev(c.row_off)

    def run():
        V, asum, dxe, da = nan(B + 1, K, D), nan(B + 1, K), nan(Pt + 1, D), nan(Pt + 1, K)
        fwd(a, xe, off, B, c.T, G, K, D, c.R, c.max_k, c2, V, asum)
        ops.nextvlad_aggregate_packed_bwd(a, xe, off, B, c.T, G, K, D, c.R, c.max_k, c2, dV, da, dxe)
        return dict(V=V, asum=asum, dxe=dxe, da=da)
    return run


@pytest.mark.parametrize("shape", vr.NX_FIXED, ids=lambda s: "x".join(str(v) for v in s))
def test_nextvlad_products_fixed_length(shape):
    """evc_nextvlad_aggregate_fwd / _bwd: V, asum, dxe, da per element."""
    c = vr.agg_case(*shape)
    rep = Report("nextvlad_aggregate")
    rep.add(c.name, vr.judge(vr.agg_ref(c), twice(_agg_fixed(c, *_agg_inputs(c)))))
    rep.done()


@pytest.mark.parametrize("shape", vr.NX_PACKED, ids=lambda s: "%dx%dx%d-%s" % (s[0], s[1], s[2], "_".join(str(k) for k in s[3])))
def test_nextvlad_products_packed(shape):
    """evc_nextvlad_aggregate_packed_fwd / _packed_fwd_mfma / _packed_bwd per element; the mfma forward is the vector forward bit for bit;
    videos without frames give exact zeros (their reference is 0 with a bound of 0); equal lengths: the fixed-length entries' bits."""
    c = vr.agg_packed_case(*shape)
    ins = _agg_inputs(c)
    refs = vr.agg_ref(c)
    got = twice(_agg_packed(c, *ins, ops.nextvlad_aggregate_packed_fwd))
    gm = twice(_agg_packed(c, *ins, ops.nextvlad_aggregate_packed_fwd_mfma))
    rep = Report("nextvlad_aggregate_packed")
    rep.add(c.name, vr.judge(refs, got))
    q = vr.judge({k: refs[k] for k in ("V", "asum")}, gm)
    for k in ("V", "asum"):
        q[k + " == vector"] = vr.exact(gm[k].view(np.uint32), got[k].view(np.uint32))
    rep.add(c.name + " mfma", q)
    for b in np.flatnonzero(np.asarray(c.ks) == 0):
        assert not got["V"][b].any() and not got["asum"][b].any() and not gm["V"][b].any() and not gm["asum"][b].any()
    if len(set(c.ks)) == 1:
        f = vr.Case()
        f.B, f.S, f.G, f.K, f.D = c.B, c.ks[0], c.G, c.K, c.D
        gf = twice(_agg_fixed(f, *ins))
        rep.add(c.name + " == fixed", {k: vr.exact(gf[k].view(np.uint32), got[k].view(np.uint32)) for k in got})
    rep.done()


# ---------------------------------------------------------------------------- assignment / softmax
@pytest.mark.parametrize("K", vr.ASSIGN_KS)
def test_nextvlad_assign(K):
    """evc_nextvlad_assign_fwd / _bwd: a, dz, datt per element, the bf16 datt at its own row stride == bf16 of the f32 datt."""
    rep = Report("nextvlad_assign")
    for G in vr.ASSIGN_GS:
        for wb in (True, False):
            c = vr.assign_case(K, G, wb)
            R = c.R
            act, da, attl = dev(c.act.reshape(R, G * K)), dev(c.da.reshape(R, G * K)), dev(c.attl)
            st = [dev(v) for v in (c.mean, c.var, c.gamma, c.beta)]
            bias = dev(c.att_bias) if wb else None

            def run():
                a, dz, datt, bf = nan(R + 1, G, K), nan(R + 1, G, K), nan(R + 1, G), nan(R + 1, c.ld_bf, dtype=BF16)
                ops.nextvlad_assign_fwd(act, R, G, K, *st, attl, a, att_bias=bias)
                ops.nextvlad_assign_bwd(act, R, G, K, *st, attl, da, dz, datt, att_bias=bias, datt_logit_bf16=bf)
                return dict(a=a, dz=dz, datt=datt, datt_bf=bf)
            got = twice(run)
            refs = vr.assign_ref(c)
            q = vr.judge({k: refs[k] for k in ("a", "dz", "datt")}, got)
            q["datt_bf"] = vr.bits_vs(got["datt_bf"], got["datt"][:R])
            rep.add(c.name, q)
    rep.done()


@pytest.mark.parametrize("K", vr.NV_SOFTMAX_KS)
def test_netvlad_softmax(K):
    c = vr.nv_softmax_case(K)
    R = c.R
    a_in = vr.softmax_f32(c.act, c.mean, c.var, c.gamma, c.beta)
    act, da, ain = dev(c.act), dev(c.da), dev(a_in)
    st = [dev(v) for v in (c.mean, c.var, c.gamma, c.beta)]

    def run():
        a, dz = nan(R + 1, K), nan(R + 1, K)
        ops.netvlad_softmax_fwd(act, R, K, *st, a)
        ops.netvlad_softmax_bwd(ain, da, R, K, dz)
        return dict(a=a, dz=dz)
    rep = Report("netvlad_softmax")
    rep.add(c.name, vr.judge(vr.nv_softmax_ref(c, a_in), twice(run)))
    rep.done()


# ---------------------------------------------------------------------------- NeXtVLAD elementwise and reductions
def test_nextvlad_normalize():
    rep = Report("nextvlad_normalize")
    for s in vr.NX_NORM_SHAPES:
        c = vr.nx_norm_case(*s)
        B, K, D = s
        V, dU, nrm = dev(c.V), dev(c.dU), dev(c.nrm)

        def run():
            Uo, norms, dV = nan(B + 1, K, D), nan(B + 1, K), nan(B + 1, K, D)
            ops.nextvlad_normalize_fwd(V, B, K, D, Uo, norms)
            ops.nextvlad_normalize_bwd(V, nrm, dU, B, K, D, dV)
            return dict(U=Uo, norms=norms, dV=dV)
        got = twice(run)
        assert not got["U"][0, 0].any() and got["norms"][0, 0] == F32(1e-12) and got["norms"][0, 1] == F32(1e-12)
        rep.add(c.name, vr.judge(vr.nx_norm_ref(c), got))
    rep.done()


@pytest.mark.parametrize("n", vr.GATE_NS)
def test_nextvlad_gate(n):
    """evc_nextvlad_gate_fwd, _gate_bwd (f32 + bf16 dgl, and the bf16 alone), _gate_bwd_add (dout2 given: per element; None: gate_bwd's bits)."""
    c = vr.gate_case(n)
    h, gl, dout, dout2 = dev(c.h), dev(c.gl), dev(c.dout), dev(c.dout2)

    def run(d2, add):
        def go():
            out, dh, dgl, bf, dh2, bfa = nan(n + 16), nan(n + 16), nan(n + 16), nan(n + 16, dtype=BF16), nan(n + 16), nan(n + 16, dtype=BF16)
            ops.nextvlad_gate_fwd(h, gl, out[:n])
            if add:
                ops.nextvlad_gate_bwd_add(h, gl, dout, d2, dh[:n], dgl=dgl[:n], dgl_bf16=bf[:n])
                ops.nextvlad_gate_bwd_add(h, gl, dout, d2, dh2[:n], dgl_bf16=bfa[:n])
            else:
                ops.nextvlad_gate_bwd(h, gl, dout, dh[:n], dgl=dgl[:n], dgl_bf16=bf[:n])
                ops.nextvlad_gate_bwd(h, gl, dout, dh2[:n], dgl_bf16=bfa[:n])
            return dict(out=out, dh=dh, dgl=dgl, dgl_bf=bf, dh_alone=dh2, dgl_bf_alone=bfa)
        return go
    rep = Report("nextvlad_gate")
    plain = twice(run(None, False))
    for tag, got, d2 in (("", plain, False), (" add(None)", twice(run(None, True)), False), (" add", twice(run(dout2, True)), True)):
        q = vr.judge(vr.gate_ref(c, d2), got)
        q["dgl_bf"] = vr.bits_vs(got["dgl_bf"], got["dgl"][:n])
        q["dgl_bf_alone == dgl_bf"] = vr.exact(got["dgl_bf_alone"], got["dgl_bf"])
        q["dh_alone == dh"] = vr.exact(got["dh_alone"].view(np.uint32), got["dh"].view(np.uint32))
        if tag == " add(None)":
            for k in got:
                q[k + " == gate_bwd"] = vr.exact(got[k].view(np.uint16 if got[k].dtype == np.uint16 else np.uint32),
                                                 plain[k].view(np.uint16 if plain[k].dtype == np.uint16 else np.uint32))
        rep.add(c.name + tag, q)
    rep.done()


def test_nextvlad_center_cast_bias_logits_wgrad_uncenter():
    rep = Report("nextvlad_center_cast")
    for s in vr.CENTER_SHAPES:
        c = vr.center_case(*s)
        xe, be = dev(c.xe), dev(c.be)

        def run():
            out = nan(c.R + 1, c.E, dtype=BF16)
            ops.nextvlad_center_cast(xe, c.R, c.E, be, out[:c.R])
            return dict(out=out)
        got = twice(run)
        q = vr.judge(vr.center_ref(c), got)
        q["out == bf16(f32)"] = vr.bits_vs(got["out"], c.xe - c.be)
        rep.add(c.name, q)
    rep.done()
    rep = Report("nextvlad_bias_logits")
    for s in vr.BIAS_SHAPES:
        for wa in (True, False):
            c = vr.bias_case(*s, wa)
            be, W, add = dev(c.be), dev(c.W), dev(c.add) if wa else None

            def run():
                out = nan(c.n_out + 16)
                ops.nextvlad_bias_logits(be, W, c.N, c.E, out[:c.n_out], add=add)
                return dict(out=out)
            got = twice(run)
            assert not got["out"][c.N:c.n_out].any()
            rep.add(c.name, vr.judge(vr.bias_ref(c), got))
    rep.done()
    rep = Report("nextvlad_wgrad_uncenter")
    for s in vr.UNCENTER_SHAPES:
        c = vr.uncenter_case(*s)
        dWc, du, be = dev(c.dWc), dev(c.du), dev(c.be)

        def run():
            dW = nan(c.N + 1, c.E)
            ops.nextvlad_wgrad_uncenter(dWc, du, be, c.N, c.E, dW)
            return dict(dW=dW)
        rep.add(c.name, vr.judge(vr.uncenter_ref(c), twice(run)))
    rep.done()


def test_nextvlad_colsum():
    """Both paths; ws=None on a tall input (the single pass) goes past ops.nextvlad_colsum, which would allocate the scratch itself."""
    rep = Report("nextvlad_colsum")
    for s in vr.COLSUM_CASES:
        c = vr.colsum_case(*s)
        x = dev(c.x)

        def run():
            out = nan(c.C + 16)
            ws = nan(vr.CS_PARTS * c.C) if c.ws else None
            _lib.call("evc_nextvlad_colsum", x.data_ptr(), c.ld, c.R, c.C, out.data_ptr(), ws.data_ptr() if c.ws else None,
                      ws.numel() if c.ws else 0, torch.cuda.current_stream().cuda_stream)
            return dict(out=out)
        rep.add(c.name, vr.judge(vr.colsum_ref(c), twice(run)))
    rep.done()


# ---------------------------------------------------------------------------- NetVLAD
@pytest.mark.parametrize("shape", vr.NV_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_netvlad_aggregate_and_normalize(shape):
    B, S, K, F = shape
    c = vr.nv_case(*shape)
    a, r, c2, dV = dev(c.a), dev(c.r), dev(c.c2), dev(c.dV)
    st = [dev(v) for v in (c.mean, c.var, c.gamma, c.beta)]

    def run():
        V, asum, da, dx = nan(B + 1, K, F), nan(B + 1, K), nan(B + 1, S, K), nan(B + 1, S, F)
        ops.netvlad_aggregate_fwd(a, r, B, S, K, F, *st, c2, V, asum)
        ops.netvlad_aggregate_bwd(a, r, B, S, K, F, *st, c2, dV, da, dx)
        return dict(V=V, asum=asum, da=da, dx=dx)
    rep = Report("netvlad_aggregate")
    refs = vr.nv_agg_ref(c)
    rep.add(c.name, vr.judge({k: refs[k] for k in ("V", "asum", "dx", "da")}, twice(run)))
    rep.done()
    c = vr.nv_norm_case(*shape)
    V, dY, n1, n2 = dev(c.V), dev(c.dY), dev(c.n1), dev(c.n2)

    def run2():
        o1, o2, Y, Yb, dVo = nan(B + 1, K), nan(B + 1), nan(B + 1, K, F), nan(B + 1, K, F, dtype=BF16), nan(B + 1, K, F)
        ops.netvlad_normalize_fwd(V, B, K, F, o1, o2, Yb, Y_f32=Y)
        ops.netvlad_normalize_bwd(V, n1, n2, dY, B, K, F, dVo)
        return dict(n1=o1, n2=o2, Y=Y, Y_bf=Yb, dV=dVo)
    got = twice(run2)
    assert not got["Y"][0, 1].any() and (B == 1 or not got["Y"][B - 1].any())
    rep = Report("netvlad_normalize")
    q = vr.judge(vr.nv_norm_ref(c), got)
    q["Y_bf"] = vr.bits_vs(got["Y_bf"], got["Y"][:B])
    rep.add(c.name, q)
    rep.done()


@pytest.mark.parametrize("shape", vr.NV_DC_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_netvlad_dcenters(shape):
    B, K, F = shape
    c = vr.nv_dc_case(*shape)
    asum, dV = dev(c.asum), dev(c.dV)

    def run():
        dc2 = nan(K + 1, F)
        ops.netvlad_dcenters(asum, dV, B, K, F, dc2)
        return dict(dc2=dc2)
    rep = Report("netvlad_dcenters")
    rep.add(c.name, vr.judge(vr.nv_dc_ref(c), twice(run)))
    rep.done()
