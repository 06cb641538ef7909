"""Guard-band and poison sweep over every pointer-taking entry point of the C ABI (include/curl_hip.h, curl_hip_grad.h).

One row of ROWS per entry point and variant (nullable outputs present and NULL, mask kinds, the flags that select another
kernel, the two slab entries with rows above and below the slab, knot counts 2 / 16 / uneven / 256).  Every row runs at its
shapes, at both alignment classes and under both poison patterns (tests/guard_arena.py): all buffers of the call sit in ONE
allocation, exactly as long as the header (or the *_bytes function) says, between two 256 KiB poisoned bands.  The raw ABI is
called with arena addresses -- the Python surface allocates its own outputs and scratch, in blocks that are larger anyway.

After the call: no guard byte changed, no input changed, no ASSIGNED output element still holds poison, rows outside a slab keep
their poison byte for byte, and the outputs of the pattern-A and the pattern-B run are bit-identical.  Then the VALUE check ties
the sweep to the references the rest of the suite holds the Python surface to: the pattern-A outputs equal ops.* on the same data
in tensors of the same alignment class, bit for bit (same kernels, same launch plan, fixed-order reductions).

What this cannot see: an out-of-bounds LOAD that does not reach a result.

tests/test_guard_arena.py (CPU) checks the helper against planted defects and that ROWS covers every pointer-taking function of
curl_amd/_lib.py's SIGNATURES and SIGNATURES_GRAD.

Measured on one MI355X: 2 574 cases (261 rows x their shapes x 2 alignment classes, both poison patterns inside each case)
in 6.6 to 8.7 s of pytest wall time over three runs, 3 ms a case (the arenas are filled on the device: only the inputs, a few
tens of KB, cross the bus); no guard, input, assignment, poison-independence or value failure.
"""
import zlib

import pytest
import torch

from curl_amd import _lib
from guard_arena import IN, INOUT, OUT, WORK, Buf, CLASSES, run_both

F32, F64, U8 = torch.float32, torch.float64, torch.uint8

# ------------------------------------------------------------------ shapes and knot counts
S6 = [(1, 1, 1), (2, 7, 9), (1, 33, 65), (2, 36, 40), (3, 16, 17), (1, 3, 1030)]
POLY = S6 + [(1, 2, 4100)]
SLAB = [s for s in S6 if s[1] >= 3]          # row0 > 0 and row0 + rows < H need three rows
KSH = [(2, 7, 9), (2, 36, 40)]               # knot-count variants: one scalar-only plane, one float4 plane of several blocks
K256SH = [(2, 36, 40)]
MS = [(1, 1, 32, 32), (2, 1, 33, 47), (1, 3, 64, 80)]

# (K, K_last) of the L, R and H segment
K16 = ((16, 16), (16, 16), (16, 16))
K2 = ((2, 2), (2, 2), (2, 2))
KUNEVEN = ((5, 3), (9, 8), (7, 4))           # CURL_K_UNEVEN: torch.chunk of 13 = 5+5+3, 26 = 9+9+8, 25 = 7+7+7+4 raw parameters
K256 = ((256, 256), (256, 256), (256, 256))
KNOTS = {"k16": K16, "k2": K2, "uneven": KUNEVEN, "k256": K256}
SEG_L, SEG_R, SEG_H = 0, 1, 2
NCURVES = (3, 3, 4)

PREP1, PREP2 = 1 << _lib.F_TUNE_PREP_SHIFT, 2 << _lib.F_TUNE_PREP_SHIFT
FLAGS = {"exact": _lib.F_EXACT_ORDER, "pwl": _lib.F_PWL, "prep1": PREP1, "prep2": PREP2, "maskfirst": _lib.F_MASK_FIRST}
MASKS = {"none": _lib.MASK_NONE, "u8": _lib.MASK_U8, "f32": _lib.MASK_F32}


def kp(k):
    return k[0] if k[0] == k[1] else k[0] | (k[1] << 16)


def n_raw(seg, k):
    return (NCURVES[seg] - 1) * k[0] + k[1]


# ------------------------------------------------------------------ data
def rand_img(g, B, C, H, W):
    return torch.rand(B, C, H, W, generator=g)


def rand_grad(g, *shape):
    return torch.randn(*shape, generator=g)


def rand_raw(g, B, seg, k):
    return torch.randn(B, n_raw(seg, k), generator=g) * 0.1


def rand_mask(g, kind, B, H, W):
    """none -> None; u8: a 0 / 1 foreground mask whose first image has its upper half masked out (whole wavefronts of zeros,
    what CURL_F_MASK_FIRST skips); f32: weights in [0, 1)."""
    if kind == "none":
        return None
    if kind == "f32":
        return torch.rand(B, 1, H, W, generator=g)
    m = (torch.rand(B, 1, H, W, generator=g) > 0.3).to(U8)
    m[0, :, :H // 2] = 0
    return m


def rand_u8(g, *shape):
    return torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(U8)


class Case:
    """bufs: the call's buffers; call(lib, A, stream) -> return code (A: the arena); surface(ops, T) -> {output name: tensor}
    from the Python surface, T = the inputs as device tensors of the row's alignment class; sel: {output name: slicer} where only
    part of an output is compared (slabs)."""

    def __init__(self, bufs, call, surface, sel=None):
        self.bufs, self.call, self.surface, self.sel = bufs, call, surface, sel or {}


class Row:
    """note: where the Python surface cannot make the row's exact launch (it always passes `reg`, never CURL_F_TUNE_PREP to the
    fused criterion forward, its own workspace under CURL_F_DIAG_SKIP_PREP) the outputs both calls produce are still compared bit
    for bit -- the header promises those variants change no bit of them -- so no row needs a tolerance."""

    def __init__(self, id, entries, shapes, make, note=""):
        self.id, self.entries, self.shapes, self.make, self.note = id, tuple(entries), shapes, make, note


ROWS = []


def row(id, entries, shapes, note=""):
    def deco(make):
        ROWS.append(Row(id, entries if isinstance(entries, (tuple, list)) else (entries,), shapes, make, note))
        return make
    return deco


def ins(**tensors):
    return [Buf(n, IN, t) for n, t in tensors.items() if t is not None]


def out(name, shape, dtype=F32, keep=()):
    return Buf(name, OUT, shape=shape, dtype=dtype, keep=keep)


def work(name, nbytes, grid=None):
    return Buf(name, WORK, nbytes=nbytes, grid=grid)


def ws_buf(lib, B, n_knots):
    return work("workspace", lib.curl_workspace_bytes(B, n_knots), grid=16)


def slab_rows(H):
    r0 = max(1, H // 3)
    return r0, max(1, H // 2)


def slab_keep(B, C, H, W, r0, n, itemsize=4):
    """The byte ranges of a [B,C,H,W] output outside rows [r0, r0 + n)."""
    keep = []
    for p in range(B * C):
        base = p * H * W * itemsize
        keep += [(base, base + r0 * W * itemsize), (base + (r0 + n) * W * itemsize, base + H * W * itemsize)]
    return keep


# ------------------------------------------------------------------ curves.py: apply_curve, adjust_*
def _apply_curve(flags, with_reg, K):
    def make(shape, g, lib):
        B, H, W = shape
        img, C = rand_img(g, B, 3, H, W), torch.exp(torch.randn(B, K, generator=g) * 0.1)
        bufs = ins(img=img, C=C) + [out("out", (B, 3, H, W))]
        if with_reg:  # += by contract: holds a set value
            bufs.append(Buf("reg", INOUT, 0.5 + torch.arange(B, dtype=F32)))

        def call(lib, A, s):
            return lib.curl_apply_curve_f32(A.ptr("img"), A.ptr("C"), A.ptr("out"), A.ptr("reg"), B, H, W, K, 1, 2, flags, s)

        def surface(ops, T):
            o, r = ops.apply_curve(T["img"], T["C"], T.get("reg"), 1, 2, flags=flags)
            return {"out": o, "reg": r} if with_reg else {"out": o}
        return Case(bufs, call, surface)
    return make


for fname, f in (("affine", 0), ("exact", _lib.F_EXACT_ORDER), ("pwl", _lib.F_PWL)):
    for rname, wr in (("reg", True), ("noreg", False)):
        row(f"apply_curve-{fname}-{rname}", "curl_apply_curve_f32", S6)(_apply_curve(f, wr, 16))
row("apply_curve-k2", "curl_apply_curve_f32", KSH)(_apply_curve(0, True, 2))
row("apply_curve-k256", "curl_apply_curve_f32", K256SH)(_apply_curve(0, True, 256))


def _adjust(name, seg, flags, with_reg, k):
    fn = f"curl_adjust_{name}_f32"

    def make(shape, g, lib):
        B, H, W = shape
        img, raw = rand_img(g, B, 3, H, W), rand_raw(g, B, seg, k)
        bufs = ins(img=img, raw=raw) + [out("out", (B, 3, H, W))] + ([out("reg", (B,))] if with_reg else [])
        bufs.append(ws_buf(lib, B, raw.shape[1]))

        def call(lib, A, s):
            return getattr(lib, fn)(A.ptr("img"), A.ptr("raw"), A.ptr("out"), A.ptr("reg"), A.ptr("workspace"),
                                    A.nbytes("workspace"), B, H, W, kp(k), flags, s)

        def surface(ops, T):
            o, r = getattr(ops, f"adjust_{name}")(T["img"], T["raw"], flags)
            return {"out": o, "reg": r} if with_reg else {"out": o}
        return Case(bufs, call, surface)
    return make


for name, seg in (("rgb", SEG_R), ("lab", SEG_L), ("hsv", SEG_H)):
    e = f"curl_adjust_{name}_f32"
    for fname in ("affine", "exact", "pwl", "prep1", "prep2"):
        row(f"adjust_{name}-{fname}", e, S6)(_adjust(name, seg, FLAGS.get(fname, 0), True, K16[seg]))
    row(f"adjust_{name}-noreg", e, S6)(_adjust(name, seg, 0, False, K16[seg]))
    for kname, shapes in (("k2", KSH), ("uneven", KSH), ("k256", K256SH)):
        row(f"adjust_{name}-{kname}", e, shapes)(_adjust(name, seg, 0, True, KNOTS[kname][seg]))
    row(f"adjust_{name}-pwl-k256", e, K256SH)(_adjust(name, seg, _lib.F_PWL, True, K256[seg]))


# ------------------------------------------------------------------ colors.py: the converters and their backwards
def _convert(name, flags=0):
    def make(shape, g, lib):
        B, H, W = shape
        bufs = ins(img=rand_img(g, B, 3, H, W)) + [out("out", (B, 3, H, W))]

        def call(lib, A, s):
            return getattr(lib, f"curl_{name}_f32")(A.ptr("img"), A.ptr("out"), B, H, W, flags, s)
        return Case(bufs, call, lambda ops, T: {"out": getattr(ops, name)(T["img"], flags)})
    return make


def _convert_bwd(name):
    def make(shape, g, lib):
        B, H, W = shape
        bufs = ins(img=rand_img(g, B, 3, H, W), grad_out=rand_grad(g, B, 3, H, W)) + [out("grad_in", (B, 3, H, W))]

        def call(lib, A, s):
            return getattr(lib, f"curl_{name}_bwd_f32")(A.ptr("img"), A.ptr("grad_out"), A.ptr("grad_in"), B, H, W, 0, s)
        return Case(bufs, call, lambda ops, T: {"grad_in": getattr(ops, name + "_backward")(T["img"], T["grad_out"])})
    return make


for name in ("rgb2lab", "lab2rgb", "rgb2hsv", "hsv2rgb"):
    row(name, f"curl_{name}_f32", S6)(_convert(name))
    row(name + "_bwd", f"curl_{name}_bwd_f32", S6)(_convert_bwd(name))
for tname in ("unroll1", "unroll4", "block64"):
    row(f"rgb2lab-tune_{tname}", "curl_rgb2lab_f32", S6)(_convert("rgb2lab", (1 << _lib.F_TUNE_UNROLL_SHIFT) if tname == "unroll1" else
                                                                 (4 << _lib.F_TUNE_UNROLL_SHIFT) if tname == "unroll4" else
                                                                 (2 << _lib.F_TUNE_BLOCK_SHIFT)))


# ------------------------------------------------------------------ model.py: the fused stages
def _stage(name, seg, mkind, flags, with_reg, k):
    fn = f"curl_{name}_stage_f32"

    def make(shape, g, lib):
        B, H, W = shape
        img, raw, mask = rand_img(g, B, 3, H, W), rand_raw(g, B, seg, k), rand_mask(g, mkind, B, H, W)
        bufs = ins(img=img, mask=mask, raw=raw) + [out("out", (B, 3, H, W))] + ([out("reg", (B,))] if with_reg else [])
        bufs.append(ws_buf(lib, B, raw.shape[1]))

        def call(lib, A, s):
            return getattr(lib, fn)(A.ptr("img"), A.ptr("mask"), MASKS[mkind], A.ptr("raw"), A.ptr("out"), A.ptr("reg"),
                                    A.ptr("workspace"), A.nbytes("workspace"), B, H, W, kp(k), flags, s)

        def surface(ops, T):
            o, r = getattr(ops, f"{name}_stage")(T["img"], T.get("mask"), T["raw"], flags=flags)
            return {"out": o, "reg": r} if with_reg else {"out": o}
        return Case(bufs, call, surface)
    return make


for name, seg, extra in (("lab", SEG_L, ("exact", "pwl")), ("hsv", SEG_H, ())):
    e = f"curl_{name}_stage_f32"
    for mk in MASKS:
        row(f"{name}_stage-mask_{mk}", e, S6)(_stage(name, seg, mk, 0, True, K16[seg]))
    row(f"{name}_stage-maskfirst", e, S6)(_stage(name, seg, "u8", _lib.F_MASK_FIRST, True, K16[seg]))
    for fname in extra + ("prep1", "prep2"):
        row(f"{name}_stage-{fname}", e, S6)(_stage(name, seg, "f32", FLAGS[fname], True, K16[seg]))
    row(f"{name}_stage-noreg", e, S6)(_stage(name, seg, "u8", 0, False, K16[seg]))
    for kname, shapes in (("k2", KSH), ("uneven", KSH), ("k256", K256SH)):
        row(f"{name}_stage-{kname}", e, shapes)(_stage(name, seg, "u8", 0, True, KNOTS[kname][seg]))
# the tuning fields pick other instantiations of the same streaming skeleton (groups per lane, block size, tile mapping, plain
# loads and stores, an LDS reservation): other tail arithmetic, the same results
TUNE = {"unroll1": 1 << _lib.F_TUNE_UNROLL_SHIFT, "unroll2": 2 << _lib.F_TUNE_UNROLL_SHIFT, "unroll4": 4 << _lib.F_TUNE_UNROLL_SHIFT,
        "block128": 1 << _lib.F_TUNE_BLOCK_SHIFT, "block64": 2 << _lib.F_TUNE_BLOCK_SHIFT, "no_nt": _lib.F_TUNE_NO_NT,
        "occ2": 2 << _lib.F_TUNE_OCC_SHIFT, "unroll4-block64": (4 << _lib.F_TUNE_UNROLL_SHIFT) | (2 << _lib.F_TUNE_BLOCK_SHIFT)}
XCD = 2 << _lib.F_TUNE_XCD_SHIFT
XCDSH = [(2, 257, 260)]  # the XCD-contiguous mapping applies from 64 workgroups per image: 66 float4 ones, 262 scalar ones
for tname, tflags in TUNE.items():
    row(f"hsv_stage-tune_{tname}", "curl_hsv_stage_f32", S6)(_stage("hsv", SEG_H, "u8", tflags, True, K16[SEG_H]))
row("hsv_stage-tune_xcd", "curl_hsv_stage_f32", XCDSH)(_stage("hsv", SEG_H, "u8", XCD, True, K16[SEG_H]))
row("hsv_stage-tune_xcd-unroll1", "curl_hsv_stage_f32", XCDSH)(_stage("hsv", SEG_H, "f32", XCD | TUNE["unroll1"], True, K16[SEG_H]))
row("lab_stage-pwl-k256", "curl_lab_stage_f32", K256SH)(_stage("lab", SEG_L, "u8", _lib.F_PWL, True, K256[SEG_L]))


# ------------------------------------------------------------------ model.py: the fused layer, forward
def _layer_inputs(g, B, H, W, mkind, ks):
    return dict(img=rand_img(g, B, 3, H, W), mask=rand_mask(g, mkind, B, H, W), rawL=rand_raw(g, B, SEG_L, ks[0]),
                rawR=rand_raw(g, B, SEG_R, ks[1]), rawH=rand_raw(g, B, SEG_H, ks[2]))


def _n_knots(ks):
    return sum(n_raw(i, ks[i]) for i in range(3))


def _layer_fwd(mkind, flags, with_reg, ks, diag=None, slab=False):
    def make(shape, g, lib):
        B, H, W = shape
        d = _layer_inputs(g, B, H, W, mkind, ks)
        r0, n = slab_rows(H) if slab else (0, H)
        keep = slab_keep(B, 3, H, W, r0, n) if slab else ()
        if diag == "no_mem":  # stores suppressed: the output buffer is left untouched
            keep = [(0, B * 3 * H * W * 4)]
        bufs = ins(**d) + [out("out", (B, 3, H, W), keep=keep)]
        if with_reg:  # CURL_F_DIAG_SKIP_PREP: `reg` is not written
            bufs.append(out("reg", (B,), keep=[(0, 4 * B)] if diag == "skip_prep" else ()))
        if diag == "skip_prep":  # the earlier call that fills the workspace writes these
            bufs += [out("fwd_out", (B, 3, H, W)), out("fwd_reg", (B,))]
        bufs.append(ws_buf(lib, B, _n_knots(ks)))
        dflags = {None: 0, "no_mem": _lib.F_DIAG_NO_MEM, "skip_prep": _lib.F_DIAG_SKIP_PREP}[diag]

        def one(lib, A, s, o, r, fl):
            head = (A.ptr("img"), A.ptr("mask"), MASKS[mkind], A.ptr("rawL"), A.ptr("rawR"), A.ptr("rawH"), A.ptr(o), A.ptr(r),
                    A.ptr("workspace"), A.nbytes("workspace"), B, H, W)
            tail = (kp(ks[0]), kp(ks[1]), kp(ks[2]), fl, s)
            if slab:
                return lib.curl_layer_fwd_slab_f32(*head, r0, n, *tail)
            return lib.curl_layer_fwd_f32(*head, *tail)

        def call(lib, A, s):
            if diag == "skip_prep":
                rc = one(lib, A, s, "fwd_out", "fwd_reg", flags)
                if rc:
                    return rc
            return one(lib, A, s, "out", "reg", flags | dflags)

        def surface(ops, T):
            args = (T["img"], T.get("mask"), T["rawL"], T["rawR"], T["rawH"])
            if slab:
                o, r = ops.curl_layer_forward_rows(*args, (r0, r0 + n), torch.zeros_like(T["img"]), flags=flags)
            else:
                o, r = ops.curl_layer_forward(*args, flags=flags | (dflags & _lib.F_DIAG_NO_MEM))
            res = {} if diag == "no_mem" else {"out": o}
            if with_reg and diag != "skip_prep":
                res["reg"] = r
            if diag == "skip_prep":
                res["fwd_out"], res["fwd_reg"] = o, r
            return res
        return Case(bufs, call, surface, {"out": lambda t: t[:, :, r0:r0 + n]} if slab else None)
    return make


E = "curl_layer_fwd_f32"
for mk in MASKS:
    row(f"layer_fwd-mask_{mk}", E, S6)(_layer_fwd(mk, 0, True, K16))
row("layer_fwd-maskfirst", E, S6)(_layer_fwd("u8", _lib.F_MASK_FIRST, True, K16))
for fname in ("exact", "pwl", "prep1", "prep2"):
    row(f"layer_fwd-{fname}", E, S6)(_layer_fwd("f32", FLAGS[fname], True, K16))
for tname, tflags in TUNE.items():
    row(f"layer_fwd-tune_{tname}", E, S6)(_layer_fwd("u8", tflags, True, K16))
row("layer_fwd-tune_xcd", E, XCDSH)(_layer_fwd("u8", XCD, True, K16))
row("layer_fwd-tune_xcd-maskfirst", E, XCDSH)(_layer_fwd("u8", XCD | _lib.F_MASK_FIRST, True, K16))
row("layer_fwd-noreg", E, S6)(_layer_fwd("u8", 0, False, K16))
for kname, shapes in (("k2", KSH), ("uneven", KSH), ("k256", K256SH)):
    row(f"layer_fwd-{kname}", E, shapes)(_layer_fwd("u8", 0, True, KNOTS[kname]))
row("layer_fwd-pwl-k256", E, K256SH)(_layer_fwd("u8", _lib.F_PWL, True, K256))
row("layer_fwd-diag_no_mem", E, KSH, note="expectation: `out` keeps its poison; reg and the workspace are written")(
    _layer_fwd("u8", 0, True, K16, diag="no_mem"))
row("layer_fwd-diag_skip_prep", E, KSH, note="expectation: `reg` keeps its poison; the workspace is an earlier call's; `out` equals "
    "the plain forward's bit for bit")(_layer_fwd("u8", 0, True, K16, diag="skip_prep"))
E = "curl_layer_fwd_slab_f32"
for mk in ("none", "u8", "f32"):
    row(f"layer_fwd_slab-mask_{mk}", E, SLAB)(_layer_fwd(mk, 0, True, K16, slab=True))
row("layer_fwd_slab-maskfirst", E, SLAB)(_layer_fwd("u8", _lib.F_MASK_FIRST, True, K16, slab=True))
row("layer_fwd_slab-pwl", E, SLAB)(_layer_fwd("f32", _lib.F_PWL, True, K16, slab=True))
row("layer_fwd_slab-exact", E, SLAB)(_layer_fwd("f32", _lib.F_EXACT_ORDER, True, K16, slab=True))
row("layer_fwd_slab-noreg", E, SLAB)(_layer_fwd("u8", 0, False, K16, slab=True))
row("layer_fwd_slab-prep1", E, SLAB)(_layer_fwd("u8", PREP1, True, K16, slab=True))
row("layer_fwd_slab-prep2", E, SLAB)(_layer_fwd("u8", PREP2, True, K16, slab=True))
row("layer_fwd_slab-tune_unroll4", E, SLAB)(_layer_fwd("u8", TUNE["unroll4"], True, K16, slab=True))
row("layer_fwd_slab-tune_xcd", E, XCDSH)(_layer_fwd("u8", XCD, True, K16, slab=True))
row("layer_fwd_slab-uneven", E, KSH)(_layer_fwd("u8", 0, True, KUNEVEN, slab=True))
row("layer_fwd_slab-k256", E, K256SH)(_layer_fwd("u8", 0, True, K256, slab=True))


def _layer_u8(mkind, white, with_reg, ks):
    def make(shape, g, lib):
        B, H, W = shape
        d = _layer_inputs(g, B, H, W, mkind, ks)
        d["img"] = rand_u8(g, B, H, W, 3)
        d["white_mask"] = rand_u8(g, B, H, W) if white else None
        bufs = ins(**d) + [out("out", (B, H, W, 3), U8)] + ([out("reg", (B,))] if with_reg else [])
        bufs.append(ws_buf(lib, B, _n_knots(ks)))

        def call(lib, A, s):
            return lib.curl_layer_fwd_u8hwc(A.ptr("img"), A.ptr("mask"), MASKS[mkind], A.ptr("rawL"), A.ptr("rawR"), A.ptr("rawH"),
                                            A.ptr("white_mask"), A.ptr("out"), A.ptr("reg"), A.ptr("workspace"),
                                            A.nbytes("workspace"), B, H, W, kp(ks[0]), kp(ks[1]), kp(ks[2]), 0, s)

        def surface(ops, T):
            o, r = ops.curl_layer_forward_u8hwc(T["img"], T.get("mask"), T["rawL"], T["rawR"], T["rawH"], T.get("white_mask"))
            return {"out": o, "reg": r} if with_reg else {"out": o}
        return Case(bufs, call, surface)
    return make


E = "curl_layer_fwd_u8hwc"
for mk, white in (("none", True), ("u8", False), ("f32", True), ("u8", True), ("none", False)):
    row(f"layer_fwd_u8hwc-mask_{mk}-{'white' if white else 'nowhite'}", E, S6)(_layer_u8(mk, white, True, K16))
row("layer_fwd_u8hwc-noreg", E, S6)(_layer_u8("u8", True, False, K16))
for kname, shapes in (("k2", KSH), ("uneven", KSH), ("k256", K256SH)):
    row(f"layer_fwd_u8hwc-{kname}", E, shapes)(_layer_u8("u8", True, True, KNOTS[kname]))


# ------------------------------------------------------------------ the fused layer, backward (affine and piecewise-linear)
def _layer_bwd(pwl, mkind, flags, with_gimg, with_greg, ks, ws_ready=False):
    fn = "curl_layer_pwl_bwd_f32" if pwl else "curl_layer_bwd_f32"
    fwd_flags = _lib.F_PWL if pwl else 0

    def make(shape, g, lib):
        B, H, W = shape
        d = _layer_inputs(g, B, H, W, mkind, ks)
        d["grad_out"] = rand_grad(g, B, 3, H, W)
        d["grad_reg"] = rand_grad(g, B) if with_greg else None
        bufs = ins(**d) + ([out("grad_img", (B, 3, H, W))] if with_gimg else [])
        bufs += [out("grad_rawL", d["rawL"].shape), out("grad_rawR", d["rawR"].shape), out("grad_rawH", d["rawH"].shape)]
        if ws_ready:  # the forward, inside the same arena, fills the workspace
            bufs += [out("fwd_out", (B, 3, H, W)), out("fwd_reg", (B,))]
        kk = [k[0] for k in ks]
        sbytes = lib.curl_layer_pwl_bwd_scratch_bytes(B, H, W, *kk) if pwl else lib.curl_layer_bwd_scratch_bytes(B, H, W)
        bufs += [ws_buf(lib, B, _n_knots(ks)), work("scratch", sbytes, grid=16)]
        K3 = (kp(ks[0]), kp(ks[1]), kp(ks[2]))

        def call(lib, A, s):
            if ws_ready:
                rc = lib.curl_layer_fwd_f32(A.ptr("img"), A.ptr("mask"), MASKS[mkind], A.ptr("rawL"), A.ptr("rawR"), A.ptr("rawH"),
                                            A.ptr("fwd_out"), A.ptr("fwd_reg"), A.ptr("workspace"), A.nbytes("workspace"), B, H, W,
                                            *K3, fwd_flags, s)
                if rc:
                    return rc
            return getattr(lib, fn)(A.ptr("img"), A.ptr("mask"), MASKS[mkind], A.ptr("rawL"), A.ptr("rawR"), A.ptr("rawH"),
                                    A.ptr("grad_out"), A.ptr("grad_reg"), A.ptr("grad_img"), A.ptr("grad_rawL"), A.ptr("grad_rawR"),
                                    A.ptr("grad_rawH"), A.ptr("workspace"), A.nbytes("workspace"), A.ptr("scratch"),
                                    A.nbytes("scratch"), B, H, W, *K3, flags | (_lib.F_WS_READY if ws_ready else 0), s)

        def surface(ops, T):
            args = (T["img"], T.get("mask"), T["rawL"], T["rawR"], T["rawH"])
            res, ws = {}, None
            if ws_ready:
                res["fwd_out"], res["fwd_reg"], ws = ops.curl_layer_forward(*args, flags=fwd_flags, return_workspace=True)
            gi, gL, gR, gH = ops.curl_layer_backward(*args, T["grad_out"], T.get("grad_reg"), need_grad_img=with_gimg, workspace=ws,
                                                     flags=flags | fwd_flags)
            res.update(grad_rawL=gL, grad_rawR=gR, grad_rawH=gH)
            if with_gimg:
                res["grad_img"] = gi
            return res
        return Case(bufs, call, surface)
    return make


for pwl, tag in ((False, "layer_bwd"), (True, "layer_pwl_bwd")):
    E = "curl_layer_pwl_bwd_f32" if pwl else "curl_layer_bwd_f32"
    for mk in MASKS:
        row(f"{tag}-mask_{mk}", E, S6)(_layer_bwd(pwl, mk, 0, True, True, K16))
        row(f"{tag}-mask_{mk}-nogimg", E, S6)(_layer_bwd(pwl, mk, 0, False, True, K16))
    row(f"{tag}-maskfirst", E, S6)(_layer_bwd(pwl, "u8", _lib.F_MASK_FIRST, True, True, K16))
    row(f"{tag}-maskfirst-nogimg", E, S6)(_layer_bwd(pwl, "u8", _lib.F_MASK_FIRST, False, True, K16))
    row(f"{tag}-nogreg", E, S6)(_layer_bwd(pwl, "u8", 0, True, False, K16))
    row(f"{tag}-ws_ready", (E, "curl_layer_fwd_f32"), S6)(_layer_bwd(pwl, "u8", 0, True, True, K16, ws_ready=True))
    for kname, shapes in (("k2", KSH), ("uneven", KSH), ("k256", K256SH)):
        if pwl and kname == "uneven":
            continue  # CURL_K_UNEVEN is CURL_E_KNOTS in the piecewise-linear forms
        row(f"{tag}-{kname}", E, shapes)(_layer_bwd(pwl, "u8", 0, True, True, KNOTS[kname]))
    row(f"{tag}-k256-nogimg", E, K256SH)(_layer_bwd(pwl, "f32", 0, False, True, K256))


# ------------------------------------------------------------------ backward of the stand-alone curve ops and the stages
def _curve_bwd(op, seg, mkind, flags, with_gimg, with_greg, k, ws_ready=False):
    """op: adjust_rgb / adjust_lab / adjust_hsv (no mask argument) or lab_stage / hsv_stage."""
    masked = op.endswith("_stage")
    fn, fwd = f"curl_{op}_bwd_f32", f"curl_{op}_f32"

    def make(shape, g, lib):
        B, H, W = shape
        d = dict(img=rand_img(g, B, 3, H, W), mask=rand_mask(g, mkind, B, H, W) if masked else None, raw=rand_raw(g, B, seg, k),
                 grad_out=rand_grad(g, B, 3, H, W), grad_reg=rand_grad(g, B) if with_greg else None)
        bufs = ins(**d) + ([out("grad_img", (B, 3, H, W))] if with_gimg else []) + [out("grad_raw", d["raw"].shape)]
        if ws_ready:
            bufs += [out("fwd_out", (B, 3, H, W)), out("fwd_reg", (B,))]
        bufs += [ws_buf(lib, B, d["raw"].shape[1]), work("scratch", lib.curl_layer_bwd_scratch_bytes(B, H, W), grid=16)]
        mhead = lambda A: (A.ptr("mask"), MASKS[mkind]) if masked else ()  # noqa: E731

        def call(lib, A, s):
            if ws_ready:
                rc = getattr(lib, fwd)(A.ptr("img"), *mhead(A), A.ptr("raw"), A.ptr("fwd_out"), A.ptr("fwd_reg"), A.ptr("workspace"),
                                       A.nbytes("workspace"), B, H, W, kp(k), 0, s)
                if rc:
                    return rc
            return getattr(lib, fn)(A.ptr("img"), *mhead(A), A.ptr("raw"), A.ptr("grad_out"), A.ptr("grad_reg"), A.ptr("grad_img"),
                                    A.ptr("grad_raw"), A.ptr("workspace"), A.nbytes("workspace"), A.ptr("scratch"),
                                    A.nbytes("scratch"), B, H, W, kp(k), flags | (_lib.F_WS_READY if ws_ready else 0), s)

        def surface(ops, T):
            res, ws = {}, None
            margs = (T["img"], T.get("mask"), T["raw"]) if masked else (T["img"], T["raw"])
            if ws_ready:
                res["fwd_out"], res["fwd_reg"], ws = getattr(ops, "_" + op)(*margs, return_workspace=True)
            kw = dict(flags=flags) if masked else {}
            gi, gr = getattr(ops, op + "_backward")(*margs, T["grad_out"], T.get("grad_reg"), with_gimg, ws, **kw)
            res["grad_raw"] = gr
            if with_gimg:
                res["grad_img"] = gi
            return res
        return Case(bufs, call, surface)
    return make


for op, seg in (("adjust_rgb", SEG_R), ("adjust_lab", SEG_L), ("adjust_hsv", SEG_H), ("lab_stage", SEG_L), ("hsv_stage", SEG_H)):
    E = f"curl_{op}_bwd_f32"
    masked = op.endswith("_stage")
    for mk in (MASKS if masked else ("none",)):
        tag = f"{op}_bwd-mask_{mk}" if masked else f"{op}_bwd"
        row(tag, E, S6)(_curve_bwd(op, seg, mk, 0, True, True, K16[seg]))
        row(tag + "-nogimg", E, S6)(_curve_bwd(op, seg, mk, 0, False, True, K16[seg]))
    mk = "u8" if masked else "none"
    if masked:
        row(f"{op}_bwd-maskfirst", E, S6)(_curve_bwd(op, seg, "u8", _lib.F_MASK_FIRST, True, True, K16[seg]))
        row(f"{op}_bwd-maskfirst-nogimg", E, S6)(_curve_bwd(op, seg, "u8", _lib.F_MASK_FIRST, False, True, K16[seg]))
    row(f"{op}_bwd-nogreg", E, S6)(_curve_bwd(op, seg, mk, 0, True, False, K16[seg]))
    row(f"{op}_bwd-ws_ready", (E, f"curl_{op}_f32"), S6)(_curve_bwd(op, seg, mk, 0, True, True, K16[seg], ws_ready=True))
    for kname, shapes in (("k2", KSH), ("uneven", KSH), ("k256", K256SH)):
        row(f"{op}_bwd-{kname}", E, shapes)(_curve_bwd(op, seg, mk, 0, True, True, KNOTS[kname][seg]))


# ------------------------------------------------------------------ the polynomial model (tri-space) and the polynomial layers
def rand_coeffs(g, *shape):
    return torch.randn(*shape, generator=g) * 0.1


def coeffs_buf(c):
    """126 coefficients: 8-byte aligned in both classes (the header demands it); 35: a float's own alignment."""
    return Buf("coeffs", IN, c, grid=8 if c.shape[-1] == 126 else None)


def _trispace_fwd(nc, residual, slab=False):
    flags = _lib.F_RESIDUAL_ONLY if residual else 0

    def make(shape, g, lib):
        B, H, W = shape
        r0, n = slab_rows(H) if slab else (0, H)
        bufs = ins(img=rand_img(g, B, 3, H, W)) + [coeffs_buf(rand_coeffs(g, B, 3, 3, nc)),
                                                  out("out", (B, 3, H, W), keep=slab_keep(B, 3, H, W, r0, n) if slab else ())]

        def call(lib, A, s):
            if slab:
                return lib.curl_trispace_fwd_slab_f32(A.ptr("img"), A.ptr("coeffs"), A.ptr("out"), B, H, W, r0, n, nc, flags, s)
            return lib.curl_trispace_fwd_f32(A.ptr("img"), A.ptr("coeffs"), A.ptr("out"), B, H, W, nc, flags, s)

        def surface(ops, T):
            if slab:
                return {"out": ops.trispace_forward_rows(T["img"], T["coeffs"], (r0, r0 + n), torch.zeros_like(T["img"]), residual)}
            return {"out": ops.trispace_forward(T["img"], T["coeffs"], residual_only=residual)}
        return Case(bufs, call, surface, {"out": lambda t: t[:, :, r0:r0 + n]} if slab else None)
    return make


def _trispace_u8(nc, white):
    def make(shape, g, lib):
        B, H, W = shape
        bufs = ins(img=rand_u8(g, B, H, W, 3), white_mask=rand_u8(g, B, H, W) if white else None)
        bufs += [coeffs_buf(rand_coeffs(g, B, 3, 3, nc)), out("out", (B, H, W, 3), U8)]

        def call(lib, A, s):
            return lib.curl_trispace_fwd_u8hwc(A.ptr("img"), A.ptr("coeffs"), A.ptr("white_mask"), A.ptr("out"), B, H, W, nc, 0, s)
        return Case(bufs, call, lambda ops, T: {"out": ops.trispace_forward_u8hwc(T["img"], T["coeffs"], T.get("white_mask"))})
    return make


def _trispace_bwd(nc, residual):
    flags = _lib.F_RESIDUAL_ONLY if residual else 0

    def make(shape, g, lib):
        B, H, W = shape
        bufs = ins(img=rand_img(g, B, 3, H, W), grad_out=rand_grad(g, B, 3, H, W))
        bufs += [coeffs_buf(rand_coeffs(g, B, 3, 3, nc)), out("grad_coeffs", (B, 3, 3, nc)),
                 work("scratch", lib.curl_trispace_bwd_scratch_bytes(B, H, W, nc), grid=16)]

        def call(lib, A, s):
            return lib.curl_trispace_bwd_f32(A.ptr("img"), A.ptr("coeffs"), A.ptr("grad_out"), A.ptr("grad_coeffs"), A.ptr("scratch"),
                                             A.nbytes("scratch"), B, H, W, nc, flags, s)
        return Case(bufs, call,
                    lambda ops, T: {"grad_coeffs": ops.trispace_backward(T["img"], T["coeffs"], T["grad_out"], residual_only=residual)})
    return make


def _trispace_bwd_img(nc, residual):
    flags = _lib.F_RESIDUAL_ONLY if residual else 0

    def make(shape, g, lib):
        B, H, W = shape
        bufs = ins(img=rand_img(g, B, 3, H, W), grad_out=rand_grad(g, B, 3, H, W))
        bufs += [coeffs_buf(rand_coeffs(g, B, 3, 3, nc)), out("grad_img", (B, 3, H, W))]

        def call(lib, A, s):
            return lib.curl_trispace_bwd_img_f32(A.ptr("img"), A.ptr("coeffs"), A.ptr("grad_out"), A.ptr("grad_img"), B, H, W, nc,
                                                 flags, s)
        return Case(bufs, call,
                    lambda ops, T: {"grad_img": ops.trispace_backward_img(T["img"], T["coeffs"], T["grad_out"], residual_only=residual)})
    return make


POLY_SLAB = [s for s in POLY if s[1] >= 3]
for nc in (126, 35):
    for residual in (False, True):
        tag = f"nc{nc}-{'residual' if residual else 'image'}"
        row(f"trispace_fwd-{tag}", "curl_trispace_fwd_f32", POLY)(_trispace_fwd(nc, residual))
        row(f"trispace_fwd_slab-{tag}", "curl_trispace_fwd_slab_f32", POLY_SLAB)(_trispace_fwd(nc, residual, slab=True))
        row(f"trispace_bwd-{tag}", "curl_trispace_bwd_f32", POLY)(_trispace_bwd(nc, residual))
        row(f"trispace_bwd_img-{tag}", "curl_trispace_bwd_img_f32", POLY)(_trispace_bwd_img(nc, residual))
    for white in (True, False):
        row(f"trispace_fwd_u8hwc-nc{nc}-{'white' if white else 'nowhite'}", "curl_trispace_fwd_u8hwc", POLY)(_trispace_u8(nc, white))


def _poly_layer(V):
    nc = 126 if V == 5 else 35

    def make(shape, g, lib):
        B, H, W = shape
        bufs = ins(img=rand_img(g, B, V, H, W), coeffs=rand_coeffs(g, B, 3, nc)) + [out("out", (B, 3, H, W))]

        def call(lib, A, s):
            return lib.curl_poly_layer_f32(A.ptr("img"), A.ptr("coeffs"), A.ptr("out"), B, H, W, V, s)
        return Case(bufs, call, lambda ops, T: {"out": ops.poly_layer(T["img"], T["coeffs"])})
    return make


def _poly_layer_bwd(V, with_gimg, with_gcoef):
    nc = 126 if V == 5 else 35

    def make(shape, g, lib):
        B, H, W = shape
        bufs = ins(img=rand_img(g, B, V, H, W), coeffs=rand_coeffs(g, B, 3, nc), grad_out=rand_grad(g, B, 3, H, W))
        bufs += ([out("grad_img", (B, V, H, W))] if with_gimg else [])
        if with_gcoef:  # the scratch serves grad_coeffs only: without it, NULL and 0 bytes
            bufs += [out("grad_coeffs", (B, 3, nc)), work("scratch", lib.curl_poly_layer_bwd_scratch_bytes(B, H, W, V), grid=16)]

        def call(lib, A, s):
            return lib.curl_poly_layer_bwd_f32(A.ptr("img"), A.ptr("coeffs"), A.ptr("grad_out"), A.ptr("grad_img"), A.ptr("grad_coeffs"),
                                               A.ptr("scratch"), A.nbytes("scratch"), B, H, W, V, 0, s)

        def surface(ops, T):
            gi, gc = ops.poly_layer_backward(T["img"], T["coeffs"], T["grad_out"], need_img_grad=with_gimg, need_coeffs_grad=with_gcoef)
            return {k: v for k, v in (("grad_img", gi), ("grad_coeffs", gc)) if v is not None}
        return Case(bufs, call, surface)
    return make


for V in (5, 3):
    row(f"poly_layer-v{V}", "curl_poly_layer_f32", POLY)(_poly_layer(V))
    for tag, gi, gc in (("both", True, True), ("nogimg", False, True), ("nogcoeffs", True, False)):
        row(f"poly_layer_bwd-v{V}-{tag}", "curl_poly_layer_bwd_f32", POLY)(_poly_layer_bwd(V, gi, gc))


# ------------------------------------------------------------------ layout edges
def _ingress(Cin):
    def make(shape, g, lib):
        B, H, W = shape
        bufs = ins(img=rand_u8(g, B, H, W, Cin)) + [out("out", (B, 3, H, W))]
        return Case(bufs, lambda lib, A, s: lib.curl_u8hwc_to_f32chw(A.ptr("img"), A.ptr("out"), B, H, W, Cin, s),
                    lambda ops, T: {"out": ops.u8hwc_to_f32chw(T["img"])})
    return make


def _egress(mkind):
    def make(shape, g, lib):
        B, H, W = shape
        x = rand_img(g, B, 3, H, W) * 1.2 - 0.1  # some values saturate
        bufs = ins(img=x, mask=rand_mask(g, mkind, B, H, W)) + [out("out", (B, H, W, 3), U8)]
        if mkind == "none":
            return Case(bufs, lambda lib, A, s: lib.curl_f32chw_to_u8hwc(A.ptr("img"), A.ptr("out"), B, H, W, s),
                        lambda ops, T: {"out": ops.f32chw_to_u8hwc(T["img"])})
        return Case(bufs, lambda lib, A, s: lib.curl_compose_white_u8hwc(A.ptr("img"), A.ptr("mask"), MASKS[mkind], A.ptr("out"), B, H, W, s),
                    lambda ops, T: {"out": ops.compose_white_u8hwc(T["img"], T["mask"])})
    return make


row("u8hwc_to_f32chw-rgb", "curl_u8hwc_to_f32chw", S6)(_ingress(3))
row("u8hwc_to_f32chw-rgba", "curl_u8hwc_to_f32chw", S6)(_ingress(4))
row("f32chw_to_u8hwc", "curl_f32chw_to_u8hwc", S6)(_egress("none"))
row("compose_white_u8hwc-mask_u8", "curl_compose_white_u8hwc", S6)(_egress("u8"))
row("compose_white_u8hwc-mask_f32", "curl_compose_white_u8hwc", S6)(_egress("f32"))


# ------------------------------------------------------------------ metric.py and the training criterion
def _psnr(mkind):
    def make(shape, g, lib):
        B, H, W = shape
        a = rand_img(g, B, 3, H, W)
        b = a + 0.05 * torch.randn(B, 3, H, W, generator=g)
        bufs = ins(a=a, b=b, mask=rand_mask(g, mkind, B, H, W)) + [out("psnr", (B,)), work("scratch", lib.curl_psnr_scratch_bytes(B, H, W))]

        def call(lib, A, s):
            return lib.curl_psnr_f32(A.ptr("a"), A.ptr("b"), A.ptr("mask"), MASKS[mkind], A.ptr("psnr"), A.ptr("scratch"),
                                     A.nbytes("scratch"), B, H, W, 1.0, s)
        return Case(bufs, call, lambda ops, T: {"psnr": ops.psnr_per_image(T["a"], T["b"], T.get("mask"), 1.0)})
    return make


for mk in MASKS:
    row(f"psnr-mask_{mk}", "curl_psnr_f32", S6)(_psnr(mk))


def _msssim(backward, window):
    def make(shape, g, lib):
        B, C, H, W = shape
        a = rand_img(g, B, C, H, W)
        b = (a + 0.1 * torch.randn(B, C, H, W, generator=g)).clamp(0, 1)
        scratch = work("scratch", lib.curl_msssim_scratch_bytes(B, C, H, W), grid=16)
        if not backward:
            bufs = ins(a=a, b=b) + [out("ssims", (B, 5)), out("mcs", (B, 5)), scratch]

            def call(lib, A, s):
                return lib.curl_msssim_fwd_f32(A.ptr("a"), A.ptr("b"), A.ptr("ssims"), A.ptr("mcs"), A.ptr("scratch"), A.nbytes("scratch"),
                                               B, C, H, W, window, s)

            def surface(ops, T):
                ss, mc = ops.msssim_stats(T["a"], T["b"], window_size=window)
                return {"ssims": ss, "mcs": mc}
            return Case(bufs, call, surface)
        bufs = ins(a=a, b=b, g_ssims=rand_grad(g, B, 5), g_mcs=rand_grad(g, B, 5)) + [out("grad_a", (B, C, H, W)), scratch]

        def call(lib, A, s):
            return lib.curl_msssim_bwd_f32(A.ptr("a"), A.ptr("b"), A.ptr("g_ssims"), A.ptr("g_mcs"), A.ptr("grad_a"), A.ptr("scratch"),
                                           A.nbytes("scratch"), B, C, H, W, window, s)
        return Case(bufs, call,
                    lambda ops, T: {"grad_a": ops.msssim_stats_backward(T["a"], T["b"], T["g_ssims"], T["g_mcs"], window_size=window)})
    return make


for window in (11, 3):
    row(f"msssim_fwd-w{window}", "curl_msssim_fwd_f32", MS)(_msssim(False, window))
    row(f"msssim_bwd-w{window}", "curl_msssim_bwd_f32", MS)(_msssim(True, window))


def _loss_terms(mkind, want_L):
    def make(shape, g, lib):
        B, H, W = shape
        bufs = ins(pred=rand_img(g, B, 3, H, W), target=rand_img(g, B, 3, H, W), mask=rand_mask(g, mkind, B, H, W))
        bufs += [out("sums", (B, 5), F64)] + ([out("L_pred", (B, 1, H, W)), out("L_target", (B, 1, H, W))] if want_L else [])
        bufs.append(work("scratch", lib.curl_loss_terms_scratch_bytes(B, H, W)))

        def call(lib, A, s):
            return lib.curl_loss_terms_f32(A.ptr("pred"), A.ptr("target"), A.ptr("mask"), MASKS[mkind], A.ptr("sums"), A.ptr("L_pred"),
                                           A.ptr("L_target"), A.ptr("scratch"), A.nbytes("scratch"), B, H, W, s)

        def surface(ops, T):
            sums, Lp, Lt = ops.loss_term_sums(T["pred"], T["target"], T.get("mask"), want_L=want_L)
            return {"sums": sums, "L_pred": Lp, "L_target": Lt} if want_L else {"sums": sums}
        return Case(bufs, call, surface)
    return make


def _loss_terms_bwd(mkind, with_gL):
    def make(shape, g, lib):
        B, H, W = shape
        bufs = ins(pred=rand_img(g, B, 3, H, W), target=rand_img(g, B, 3, H, W), mask=rand_mask(g, mkind, B, H, W),
                   weights=rand_grad(g, 4), grad_L_pred=rand_grad(g, B, 1, H, W) if with_gL else None)
        bufs.append(out("grad_pred", (B, 3, H, W)))

        def call(lib, A, s):
            return lib.curl_loss_terms_bwd_f32(A.ptr("pred"), A.ptr("target"), A.ptr("mask"), MASKS[mkind], A.ptr("weights"),
                                               A.ptr("grad_L_pred"), A.ptr("grad_pred"), B, H, W, s)
        return Case(bufs, call, lambda ops, T: {"grad_pred": ops.loss_terms_backward(T["pred"], T["target"], T.get("mask"), T["weights"],
                                                                                    T.get("grad_L_pred"))})
    return make


for mk in MASKS:
    row(f"loss_terms-mask_{mk}", "curl_loss_terms_f32", S6)(_loss_terms(mk, True))
    row(f"loss_terms_bwd-mask_{mk}", "curl_loss_terms_bwd_f32", S6)(_loss_terms_bwd(mk, True))
row("loss_terms-noL", "curl_loss_terms_f32", S6)(_loss_terms("u8", False))
row("loss_terms_bwd-nogL", "curl_loss_terms_bwd_f32", S6)(_loss_terms_bwd("u8", False))


def _layer_loss(mkind, want_L, with_reg, ks, flags=0):
    def make(shape, g, lib):
        B, H, W = shape
        d = _layer_inputs(g, B, H, W, mkind, ks)
        d["target"] = rand_img(g, B, 3, H, W)
        bufs = ins(**d) + [out("out", (B, 3, H, W))] + ([out("reg", (B,))] if with_reg else []) + [out("sums", (B, 5), F64)]
        bufs += [out("L_pred", (B, 1, H, W)), out("L_target", (B, 1, H, W))] if want_L else []
        bufs += [ws_buf(lib, B, _n_knots(ks)), work("scratch", lib.curl_loss_terms_scratch_bytes(B, H, W))]

        def call(lib, A, s):
            return lib.curl_layer_loss_fwd_f32(A.ptr("img"), A.ptr("mask"), MASKS[mkind], A.ptr("rawL"), A.ptr("rawR"), A.ptr("rawH"),
                                               A.ptr("target"), A.ptr("out"), A.ptr("reg"), A.ptr("sums"), A.ptr("L_pred"),
                                               A.ptr("L_target"), A.ptr("workspace"), A.nbytes("workspace"), A.ptr("scratch"),
                                               A.nbytes("scratch"), B, H, W, kp(ks[0]), kp(ks[1]), kp(ks[2]), flags, s)

        def surface(ops, T):
            o, r, sums, Lp, Lt, _ = ops.layer_loss_forward(T["img"], T.get("mask"), T["rawL"], T["rawR"], T["rawH"], T["target"],
                                                           want_L=want_L)
            res = {"out": o, "sums": sums}
            if with_reg:
                res["reg"] = r
            if want_L:
                res["L_pred"], res["L_target"] = Lp, Lt
            return res
        return Case(bufs, call, surface)
    return make


E = "curl_layer_loss_fwd_f32"
for mk in MASKS:
    row(f"layer_loss_fwd-mask_{mk}", E, S6)(_layer_loss(mk, True, True, K16))
# (the surface passes flags = 0, which collapses the curves inside the kernel at these sizes; CURL_F_TUNE_PREP's placement never
# changes results -- include/curl_hip.h -- so the comparison stays bit for bit)
row("layer_loss_fwd-prep1", E, S6, note="the surface cannot ask for the separate knot-prep launch; results are bit-identical by the "
    "header's word on CURL_F_TUNE_PREP")(_layer_loss("u8", True, True, K16, PREP1))
row("layer_loss_fwd-prep2", E, S6, note="as prep1: the surface passes flags = 0 (the same in-kernel collapse at these sizes, chosen "
    "by the library instead of asked for)")(_layer_loss("f32", True, True, K16, PREP2))
row("layer_loss_fwd-noL", E, S6)(_layer_loss("u8", False, True, K16))
row("layer_loss_fwd-noreg", E, S6)(_layer_loss("u8", True, False, K16))
for kname, shapes in (("k2", KSH), ("uneven", KSH), ("k256", K256SH)):
    row(f"layer_loss_fwd-{kname}", E, shapes)(_layer_loss("u8", True, True, KNOTS[kname]))


# ------------------------------------------------------------------ the sweep
def covered_entries():
    return {e for r in ROWS for e in r.entries}


def pointer_taking_entries():
    """Every function of the two signature tables with a device-pointer argument.  (The stream, always the last argument,
    travels as the same ctypes type: it is not looked at.)"""
    table = {**_lib.SIGNATURES, **_lib.SIGNATURES_GRAD}
    return {n for n, (_, args) in table.items() if any(a is _lib._c_f for a in args[:-1])}


assert len({r.id for r in ROWS}) == len(ROWS), "duplicate row id"
PARAMS = [(r, s, c) for r in ROWS for s in r.shapes for c in CLASSES]


def _place(t, cls, dev):
    """The tensor on the device, in the alignment class: "16+4" = one element past an allocation boundary (test_gpu_parity.py's
    _misaligned)."""
    t = t.to(dev)
    if cls == "16":
        assert t.data_ptr() % 16 == 0
        return t
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def _bits(t):
    return t.contiguous().reshape(-1).view(U8)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from curl_amd import ops as _ops
    _lib.load()  # fail loudly if the HIP library is missing
    return _ops


@pytest.mark.gpu
@pytest.mark.parametrize("r,shape,cls", PARAMS, ids=[f"{r.id}-{'x'.join(map(str, s))}-{c}" for r, s, c in PARAMS])
def test_guard_bands(ops, dev, r, shape, cls):
    lib = _lib.load()
    g = torch.Generator().manual_seed(zlib.crc32(f"{r.id}-{shape}".encode()))
    case = r.make(shape, g, lib)
    stream = torch.cuda.current_stream().cuda_stream

    def call(A):
        rc = case.call(lib, A, stream)
        assert rc == 0, (rc, lib.curl_last_error().decode("utf-8", "replace"))

    A = run_both(case.bufs, cls, dev, call)
    T = {b.name: _place(b.data, cls, dev) for b in case.bufs if b.data is not None}
    with torch.no_grad():
        ref = case.surface(ops, T)
    assert ref, "the row compares nothing with the Python surface"
    for name, want in ref.items():
        got = A.read(name)
        sel = case.sel.get(name)
        if sel is not None:
            got, want = sel(got), sel(want)
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
        ne = _bits(got) != _bits(want)
        if bool(ne.any()):
            d = (got.double() - want.double()).abs()
            pytest.fail(f"value: output '{name}' differs from the Python surface in {int(ne.sum())} bytes, first at byte "
                        f"{int(torch.nonzero(ne)[0])}; max |difference| {float(d[~d.isnan()].max()) if (~d.isnan()).any() else 'nan'}")
