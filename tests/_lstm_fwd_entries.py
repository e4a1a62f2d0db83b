"""One well-formed raw call (through _lib.call, no ops wrapper) of each of the ten forward entry points of csrc/evc_lstm_fwd.hip, on seeded
operands at the smallest legal shapes.  Shared by tests/test_gpu_lstm_fwd_refusals.py (one argument broken at a time) and
scripts/fwd_entries_digest.py (sha256 of every output buffer: two builds of the library compared entry by entry).

    call = build("evc_lstm_level2_fwd", T=3, rows=[32, 16, 0])
    call.run()                      # the well-formed call
    call.run(ld_state=4 * H + 2)    # the same call with one argument replaced (by the C parameter's name)

`variant` selects the forms an entry has beyond the plain one (VARIANTS).  Outputs are prefilled with the byte 0x5A, so the elements a call
does not write (the gate records of finished rows, the slots a row plan drops) are the same bits in every run.
"""
import ctypes as C

import torch

from efficientvideoclassification_youtube8m_amd import _lib

DEV = "cuda:0"
BF16, F16, F32, U8 = torch.bfloat16, torch.float16, torch.float32, torch.uint8
FILL = 0x5A
M0, H0, KIN0 = 32, 128, 64          # the smallest legal shape of the bf16 / f16 forms
KIN8 = 384                          # e4m3 layer forms: kx8 >= 384
H_FP8_STACK = 512                   # evc_lstm_stack2_fwd_f16_fp8lo: H >= 512

ENTRIES = ("evc_lstm_layer_fwd", "evc_lstm_layer_fwd_f16", "evc_lstm_layer_fwd_f16_fp8lo", "evc_lstm_layer_fwd_f16_dith", "evc_lstm_layer_fwd_hp",
           "evc_lstm_level2_fwd", "evc_lstm_level2_fwd_high", "evc_lstm_stack2_fwd", "evc_lstm_stack2_fwd_f16", "evc_lstm_stack2_fwd_f16_fp8lo")
PLANNED = ("evc_lstm_layer_fwd", "evc_lstm_layer_fwd_f16", "evc_lstm_layer_fwd_f16_fp8lo", "evc_lstm_layer_fwd_f16_dith", "evc_lstm_level2_fwd",
           "evc_lstm_level2_fwd_high")          # the entries that take row_map / rows_per_step
VARIANTS = {                                     # beyond None (the plain form)
    "evc_lstm_layer_fwd": ("hoist",),
    "evc_lstm_layer_fwd_f16": ("wide",),
    "evc_lstm_layer_fwd_f16_fp8lo": ("hlo", "xint"),
    "evc_lstm_layer_fwd_f16_dith": ("kx8=0",),
    "evc_lstm_layer_fwd_hp": ("M=1024",),
    "evc_lstm_level2_fwd_high": ("hlo+xint",),
    "evc_lstm_stack2_fwd_f16": ("h0_ext",),
    "evc_lstm_stack2_fwd_f16_fp8lo": ("hlo",),
}


class Gen:
    def __init__(self, seed):
        self.g = torch.Generator(device="cpu").manual_seed(seed)

    def randn(self, shape, dt, scale):
        return (torch.randn(shape, generator=self.g) * scale).to(dt).to(DEV)

    def e4m3(self, shape):
        """Random OCP e4m3 bytes of magnitude < 2 (no NaN encodings)."""
        m = torch.randint(0, 0x40, shape, generator=self.g, dtype=torch.int32)
        s = torch.randint(0, 2, shape, generator=self.g, dtype=torch.int32) * 0x80
        return (m | s).to(U8).to(DEV)

    def lens(self, M, T):
        v = torch.randint(0, T + 1, (M,), generator=self.g, dtype=torch.int32)
        v[0], v[1] = T, 0
        return v.to(DEV)


def out(shape, dt, slack=0):
    """A prefilled output buffer (slack: spare elements behind it, for the calls that hand in an offset pointer)."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full(((n + slack) * torch.empty((), dtype=dt).element_size(),), FILL, dtype=U8, device=DEV).view(dt)
    return flat[:n].view(*shape)


def _arg(v):
    return v.data_ptr() if isinstance(v, torch.Tensor) else v


class Call:
    def __init__(self, name, args, outs, rings, keys):
        self.name, self.args, self.outs, self.rings, self.keys = name, args, outs, rings, keys
        # args: C parameter name -> tensor / int / None / ctypes array, in the entry's order (without the stream); outs: label -> every buffer
        # the entry writes; rings: the labels of the h buffers (what the entry clears first); keys: the names of c_state / gates / c_all

    def run(self, **over):
        a = dict(self.args)
        for k in over:
            assert k in a, (self.name, k)
        a.update(over)
        _lib.call(self.name, *[_arg(v) for v in a.values()], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()

    def refill(self):
        for t in self.outs.values():
            t.view(U8).fill_(FILL)

    def bits(self):
        torch.cuda.synchronize()
        return {k: t.contiguous().view(U8).cpu().clone() for k, t in self.outs.items()}


def _plan(g, M, T, rows):
    """(lens, row_map, rows_per_step): unplanned, or the slot-ordered lens of a plan with rows[t] live slots at step t."""
    if rows is None:
        return g.lens(M, T), None, None
    assert len(rows) == T and rows[0] <= M
    lens = torch.tensor([sum(1 for r in rows if r > i) for i in range(M)], dtype=torch.int32).to(DEV)
    row_map = torch.arange(M - 1, -1, -1, dtype=torch.int32).to(DEV)        # slot -> state row: a permutation of [0, M)
    return lens, row_map, (C.c_int32 * T)(*rows)


def _x_rows8(g, T, M, kx16, kx8, integer=False):
    """x rows of the e4m3 layer forms: [kx16 f16 | kx8 e4m3 bytes] in f16 containers; returns (x, ldx, x8_off)."""
    ldx = kx16 + kx8 // 2
    x = torch.zeros((T, M, ldx), dtype=F16, device=DEV)
    if integer:          # the integer-frame form: exact odd integers 2q - 255
        q = torch.randint(0, 256, (T, M, kx16), generator=g.g, dtype=torch.int32)
        x[..., :kx16] = (2 * q - 255).to(F16).to(DEV)
    else:
        x[..., :kx16] = g.randn((T, M, kx16), F16, 0.5)
    x.view(U8).view(T, M, 2 * ldx)[..., 2 * kx16:] = g.e4m3((T, M, kx8))
    return x, ldx, 2 * kx16


def _tape(T, M, H):
    return out((T, M, H, 2), torch.int32, slack=4), out((T + 1, M, H), BF16)


def _state(S, H, k):
    return S.data_ptr() + 4 * H * k


def build(name, T=2, M=None, rows=None, variant=None, seed=1234):
    assert name in ENTRIES and (rows is None or name in PLANNED) and (variant is None or variant in VARIANTS.get(name, ()))
    g = Gen(seed)
    M = M or (1024 if variant == "M=1024" else M0)
    H = H_FP8_STACK if name == "evc_lstm_stack2_fwd_f16_fp8lo" else H0
    lens, row_map, rps = _plan(g, M, T, rows)
    two = name.startswith(("evc_lstm_level2", "evc_lstm_stack2"))
    S = out((M, (4 if two else 2) * H), F32, slack=4)
    bias = [g.randn((4 * H,), F32, 0.1) for _ in range(2)]
    tapes = [_tape(T, M, H) for _ in range(2)]
    outs = {"S": S}
    for l in range(2 if two else 1):
        outs["gates%d" % l], outs["c_all%d" % l] = tapes[l]
    if two:
        st = dict(c_state0=_state(S, H, 0), h_state0=_state(S, H, 1), c_state1=_state(S, H, 2), h_state1=_state(S, H, 3), ld_state=4 * H)
        tp = dict(gates0=tapes[0][0], c_all0=tapes[0][1], gates1=tapes[1][0], c_all1=tapes[1][1])
        keys = dict(c_state="c_state0", gates="gates0", c_all="c_all0")
    else:
        st = dict(c_state=_state(S, H, 0), h_state=_state(S, H, 1), ld_state=2 * H)
        tp = dict(gates=tapes[0][0], c_all=tapes[0][1])
        keys = dict(c_state="c_state", gates="gates", c_all="c_all")
    plan = dict(row_map=row_map, rows_per_step=rps)
    shape = dict(T=T, M=M, H=H)
    rings = {}
    w8e = 0              # the e4m3 products count at 2^-7: they reach the stored bits

    if name == "evc_lstm_layer_fwd":
        Kin, hoist = KIN0, variant == "hoist"
        rings["hbuf"] = out((T + 1, M, H), BF16)
        zx = out((T * M, 4 * H), F32) if hoist else None
        args = dict(x=g.randn((T, M, Kin), BF16, 0.5), wT=g.randn((4 * H, Kin + H), BF16, 0.1), bias=bias[0], len=lens, T=T, M=M, Kin=Kin, H=H,
                    hoist=int(hoist), zx_ws=zx, hbuf=rings["hbuf"], **st, **tp, **plan)
    elif name == "evc_lstm_layer_fwd_f16":
        Kin, wide = KIN0, variant == "wide"
        ldh = 2 * H if wide else H
        rings["hbuf"], rings["hbuf_bf16"] = out((T + 1, M, ldh), F16), out((T + 1, M, H), BF16)
        args = dict(x=g.randn((T, M, Kin), F16, 0.5), ldx=Kin, wT=g.randn((4 * H, Kin + ldh), F16, 0.1), bias=bias[0], len=lens, T=T, M=M, Kin=Kin, H=H,
                    hbuf=rings["hbuf"], h_wide=int(wide), hbuf_bf16=rings["hbuf_bf16"], **st, **tp, **plan)
    elif name in ("evc_lstm_layer_fwd_f16_fp8lo", "evc_lstm_level2_fwd_high"):
        h_lo, xint = variant in ("hlo", "hlo+xint"), variant in ("xint", "hlo+xint")
        kx16 = kx8 = KIN8
        gap = 128 if xint else 0
        x, ldx, x8_off = _x_rows8(g, T, M, kx16, kx8, integer=xint)
        ldh = 2 * H if h_lo else 3 * H // 2
        w16 = g.randn((4 * H, kx16 + H), F16, 0.002 if xint else 0.1)
        w8 = g.e4m3((4 * H, kx8 + gap + (2 if h_lo else 1) * H))
        rs = (g.randn((T, M), F32, 0.0005).abs() + 0.001) if xint else None
        cc = g.randn((4 * H,), F32, 0.05) if xint else None
        head = dict(x=x, ldx=ldx, kx16=kx16, x8_off=x8_off, kx8=kx8)
        if name == "evc_lstm_layer_fwd_f16_fp8lo":
            rings["hbuf"], rings["hbuf_bf16"] = out((T + 1, M, ldh), F16), out((T + 1, M, H), BF16)
            args = dict(**head, wT16=w16, wT8=w8, w8_scale_exp=w8e, h_lo=int(h_lo), bias=bias[0], len=lens, **shape, hbuf=rings["hbuf"],
                        hbuf_bf16=rings["hbuf_bf16"], **st, **tp, **plan, x_row_scale=rs, x_col_const=cc, b8_gap=gap)
        else:
            w1 = g.randn((T, 4 * H, 2 * H), F16, 0.1)        # one image per step
            rings.update(hbuf0=out((T + 1, M, ldh), F16), hbuf0_bf16=out((T + 1, M, H), BF16), hbuf1=out((T + 1, M, H), F16),
                         hbuf1_bf16=out((T + 1, M, H), BF16))
            args = dict(**head, wT16_0=w16, wT8_0=w8, w8_scale_exp=w8e, h_lo=int(h_lo), bias0=bias[0], x_row_scale=rs, x_col_const=cc, b8_gap=gap,
                        wT16_1=w1, w16_step_stride=w1.stride(0), bias1=bias[1], len=lens, **shape, **rings, **st, **tp, **plan)
    elif name == "evc_lstm_layer_fwd_f16_dith":
        kx16 = KIN8
        kx8 = 0 if variant == "kx8=0" else KIN8
        x, ldx, x8_off = _x_rows8(g, T, M, kx16, kx8)
        w16 = g.randn((T, 4 * H, kx16 + H), F16, 0.1)
        rings["hbuf"], rings["hbuf_bf16"] = out((T + 1, M, H), F16), out((T + 1, M, H), BF16)
        args = dict(x=x, ldx=ldx, kx16=kx16, x8_off=x8_off, kx8=kx8, wT16=w16, w16_step_stride=w16.stride(0), wT8=g.e4m3((4 * H, kx8)) if kx8 else None,
                    ldb8=kx8, scale8_exp=7, bias=bias[0], len=lens, **shape, hbuf=rings["hbuf"], hbuf_bf16=rings["hbuf_bf16"], **st, **tp, **plan)
    elif name == "evc_lstm_layer_fwd_hp":
        Kin = KIN0
        rings["hbuf"], rings["hbuf_lohi"] = out((T + 1, M, H), BF16), out((T + 1, M, 2 * H), BF16)
        args = dict(x_lohi=g.randn((T, M, 2 * Kin), BF16, 0.5), wx_hilo=g.randn((4 * H, 2 * Kin), BF16, 0.1), ldwx=2 * Kin,
                    wh_hilo=g.randn((4 * H, 2 * H), BF16, 0.1), ldwh=2 * H, bias=bias[0], len=lens, T=T, M=M, Kin=Kin, H=H,
                    zx_ws=out((T * M, 4 * H), F32), hbuf=rings["hbuf"], hbuf_lohi=rings["hbuf_lohi"], **st, **tp)
    elif name in ("evc_lstm_level2_fwd", "evc_lstm_stack2_fwd"):
        Kin = KIN0
        rings["hbuf0"], rings["hbuf1"] = out((T + 1, M, H), BF16), out((T + 1, M, H), BF16)
        args = dict(x=g.randn((T, M, Kin), BF16, 0.5), wT0=g.randn((4 * H, Kin + H), BF16, 0.1), bias0=bias[0], wT1=g.randn((4 * H, 2 * H), BF16, 0.1),
                    bias1=bias[1], len=lens, T=T, M=M, Kin=Kin, H=H)
        if name == "evc_lstm_stack2_fwd":
            args.update(zx_ws=out((T * M, 4 * H), F32))
        args.update(**rings, **st, **tp)
        if name == "evc_lstm_level2_fwd":
            args.update(plan)
    elif name == "evc_lstm_stack2_fwd_f16":
        Kin, ext = KIN0, variant == "h0_ext"
        rings.update(h0_wide=out((T + 1, M, 2 * H), F16), h1_wide=out((T + 1, M, 2 * H), F16), hbuf0=out((T + 1, M, H), BF16),
                     hbuf1=out((T + 1, M, H), BF16))
        args = dict(x=g.randn((T, M, Kin), F16, 0.5), x_segments=1, wT0=g.randn((4 * H, Kin + (2 if ext else 1) * H), F16, 0.1), h0_ext=int(ext),
                    bias0=bias[0], wT1_wlo=g.randn((4 * H, 4 * H), F16, 0.1), bias1=bias[1], len=lens, T=T, M=M, Kin=Kin, H=H,
                    zx_ws=out((T * M, 4 * H), F32), **rings, **st, **tp)
    else:
        assert name == "evc_lstm_stack2_fwd_f16_fp8lo"
        Kin, h_lo = KIN0, variant == "hlo"
        ldh, k8 = (2 * H if h_lo else 3 * H // 2), (2 if h_lo else 1)
        rings.update(h0_rows=out((T + 1, M, ldh), F16), h1_rows=out((T + 1, M, ldh), F16), hbuf0=out((T + 1, M, H), BF16),
                     hbuf1=out((T + 1, M, H), BF16))
        args = dict(x=g.randn((T, M, Kin), F16, 0.5), x_segments=1, wT0=g.randn((4 * H, Kin + H), F16, 0.05), wT0_8=g.e4m3((4 * H, k8 * H)), bias0=bias[0],
                    wT1=g.randn((4 * H, 2 * H), F16, 0.05), wT1_8=g.e4m3((4 * H, 2 * k8 * H)), w8_scale_exp=w8e, h_lo=int(h_lo), bias1=bias[1], len=lens,
                    T=T, M=M, Kin=Kin, H=H, zx_ws=out((T * M, 4 * H), F32), **rings, **st, **tp)
    outs.update(rings)
    if args.get("zx_ws") is not None:
        outs["zx_ws"] = args["zx_ws"]
    assert len(args) + 1 == len(_lib.SIGNATURES[name]), (name, len(args) + 1, len(_lib.SIGNATURES[name]))
    return Call(name, args, outs, list(rings), keys)
