"""Tensor-level entry points: torch tensors in, HIP kernels underneath (via the C ABI).

PyTorch is plumbing here: it owns device memory (caching allocator) and the stream.
Every function enqueues on torch's CURRENT stream and returns without synchronising.
"""
import functools
from types import SimpleNamespace

import torch

from . import _lib
from ._lib import F_EXACT_ORDER, F_MASK_FIRST, F_PWL, MASK_F32, MASK_NONE, MASK_U8


def _is_empty_image(img):
    """An empty [B,3,H,W] image (B == 0 or H*W == 0): the ops answer it without a launch."""
    return isinstance(img, torch.Tensor) and img.dim() == 4 and img.shape[1] == 3 and img.numel() == 0


def _empty_ok(mask_arg=None):
    """The reference's eager ops accept empty tensors ([0,3,H,W], or H*W == 0) and return empty ones; the kernels
    are never launched on zero pixels.  Ops that also return a regulariser still owe it (it depends on the knots
    only): it is produced by the same entry point on a 1x1 stand-in image."""
    def deco(fn):
        @functools.wraps(fn)
        def wrapper(img, *args, **kwargs):
            if not _is_empty_image(img):
                return fn(img, *args, **kwargs)
            _need_device(img, "img")
            out = torch.empty_like(img)
            if mask_arg is None:          # image -> image
                return out
            B = img.shape[0]
            if B == 0:
                reg = torch.zeros(0, dtype=torch.float32, device=img.device)
            else:
                args = list(args)
                if mask_arg >= 0:
                    args[mask_arg] = None  # the mask's shape belongs to the empty image
                kwargs.pop("out", None)
                res = fn(img.new_zeros((B, 3, 1, 1)), *args, **kwargs)
                reg = res[1]
            return (out, reg, None) if kwargs.get("return_workspace") else (out, reg)
        return wrapper
    return deco


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t):
    """The raw handle of torch's current stream on the tensor's device.  torch._C._cuda_getCurrentRawStream is the direct
    accessor (what torch's own compiled-kernel launchers use): 0.2 us instead of the ~2.5 us of building a torch.cuda.Stream
    object per call -- on a 12 us launch the host side is the cost (tools/small_batch.py)."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


def _check_same_device(named):
    """Every tensor of one call must live on ONE device: a knot / mask / gradient tensor on cuda:1 next to an image on
    cuda:0 would hand the kernel a foreign pointer (a GPU fault) where the reference's eager ops raise cleanly."""
    devs = [(n, t.device) for n, t in named if isinstance(t, torch.Tensor)]
    cuda = [(n, d) for n, d in devs if d.type == "cuda"]
    if len({d for _, d in cuda}) > 1:
        raise ValueError("expected all tensors to be on the same device, got " +
                         ", ".join(f"{n} on {d}" for n, d in cuda))
    return cuda[0][1] if cuda and len(cuda) == len(devs) else None


def _one_device(fn):
    """Check that all tensor arguments share a device and run the call with that device current (the library
    enqueues on the stream it is handed and never calls hipSetDevice itself)."""
    import inspect
    params = list(inspect.signature(fn).parameters)

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        # fast path (the common call): every tensor on the CURRENT device -- nothing to switch, nothing to report
        dev = None
        for a in args:
            if isinstance(a, torch.Tensor):
                if dev is None:
                    dev = a.device
                elif a.device != dev:
                    dev = False
                    break
        if dev and not kwargs.keys() - _PLAIN_KWARGS and dev.type == "cuda" and dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        named = list(zip(params, args)) + list(kwargs.items())
        dev = _check_same_device(named)
        if dev is None:  # a CPU tensor (or none at all): the body's own checks raise the documented errors
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapper


# keyword arguments that carry no tensor, or one whose device the body checks itself against the image's (`out`: _check_out,
# `workspace`: curl_layer_backward); any other tensor passed by keyword takes the slow, fully checked path
_PLAIN_KWARGS = frozenset(("flags", "return_workspace", "residual_only", "need_grad_img", "need_img_grad", "need_coeffs_grad", "max_intensity", "window_size",
                           "want_L", "out", "workspace", "size"))


def _coeffs32(coeffs, pairs=True):
    """float32 and contiguous; pairs=True (the spatial 126-coefficient tables, which the kernels copy into LDS as 8-byte
    pairs): also 8-byte aligned -- a view that starts at an odd float of its storage is copied."""
    c = coeffs.to(torch.float32).contiguous()
    return c.clone() if pairs and c.data_ptr() % 8 else c


def _check_out(out, img):
    """A caller-supplied `out` is written in place by the kernel: anything but a contiguous float32 tensor of the
    image's shape on the image's device would be an out-of-bounds or foreign-device write."""
    if not isinstance(out, torch.Tensor):
        raise TypeError(f"out must be a torch.Tensor, got {type(out).__name__}")
    if out.shape != img.shape or out.dtype != img.dtype or not out.is_contiguous() or out.device != img.device:
        raise ValueError(f"out must be a contiguous {img.dtype} tensor of shape {tuple(img.shape)} on {img.device}, got "
                         f"{out.dtype} {tuple(out.shape)} on {out.device}"
                         f"{'' if out.is_contiguous() else ' (not contiguous)'}")
    return out


def _need_device(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(
            f"curl_amd: {name} is on {t.device}; this path runs on a HIP device only "
            "(no CPU fallback -- move the tensor to cuda)")


def _image(t, name="img"):
    _need_device(t, name)
    if t.dim() != 4 or t.shape[1] != 3:
        raise ValueError(f"{name} must be [B,3,H,W], got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if t.numel() == 0:
        raise ValueError(f"{name} is empty: {tuple(t.shape)}")
    return t.contiguous()


def _knots(t, name, ncurves, B):
    _need_device(t, name)
    if t.dim() != 2 or t.shape[0] != B:
        raise ValueError(f"{name} must be [B={B}, {ncurves}*K], got {tuple(t.shape)}")
    N = t.shape[1]
    K = -(-N // ncurves)  # torch.chunk(P, n, dim=1): chunks of ceil(N / n) (curves.py:53,105,152) ...
    if ncurves > 1 and -(-N // K) != ncurves:
        # ... of which there may then be fewer than n: the reference's tuple unpacking fails on that
        raise ValueError(f"{name}: torch.chunk splits {N} parameters into {-(-N // K)} chunks, not {ncurves} curves")
    K_last = N - (ncurves - 1) * K  # ... and the last one holds the remainder
    if K < 2 or K > _lib.MAX_KNOTS or K_last < 2:
        raise ValueError(f"{name}: {K} knots per curve ({K_last} in the last); supported range is [2, {_lib.MAX_KNOTS}]")
    # the C ABI's packed form (include/curl_hip.h CURL_K_UNEVEN): K, and the last curve's count in the high half if it differs
    if t.dtype is not torch.float32 or not t.is_contiguous():
        t = t.to(torch.float32).contiguous()
    return t, (K if K_last == K else K | (K_last << 16))


def _layer_knots(L, R, H, B):
    """The layer's three knot segments, checked and packed -> (Lc, Rc, Hc, Kl, Kr, Kh, n_knots)."""
    Lc, Kl = _knots(L, "L", 3, B)
    Rc, Kr = _knots(R, "R", 3, B)
    Hc, Kh = _knots(H, "H", 4, B)
    return Lc, Rc, Hc, Kl, Kr, Kh, Lc.shape[1] + Rc.shape[1] + Hc.shape[1]


# Coefficients per polynomial, C(V + d, d), by variable count V: orders d = 1..4.  The eight counts are all different, so a
# table's width names its order and its variable count (include/curl_hip.h).
POLY_COEFFS = {5: (6, 21, 56, 126), 3: (4, 10, 20, 35)}
# ... and the order-4 width of the same variable count: the reference's monomial order is graded (model.py:222-246), so an
# order-d table is the first n entries of the order-4 table of the same polynomial -- the backward kernels (order 4 only)
# take it zero-padded and their coefficient gradient is cut back to n
_ORDER4_WIDTH = {n: counts[3] for counts in POLY_COEFFS.values() for n in counts}


def _check_coeffs(coeffs, B):
    """The polynomial path's [B,3,3,126|35] coefficient table, or a lower order's (then converted by _coeffs32)."""
    _need_device(coeffs, "coeffs")
    if coeffs.dim() != 4 or coeffs.shape[:3] != (B, 3, 3) or coeffs.shape[3] not in _ORDER4_WIDTH:
        raise ValueError(f"coeffs must be [B={B},3,3,126|35], got {tuple(coeffs.shape)} "
                         "(orders 3, 2, 1: 56|20, 21|10, 6|4 in place of 126|35)")


def _nc_arg(n):
    """A table width as the forward entries' num_coeffs: 126 | 35 plain, a lower order's count with its order in the high half
    (include/curl_hip_poly.h)."""
    for counts in POLY_COEFFS.values():
        if n in counts[:3]:
            return _lib.poly_coeffs(n, counts.index(n) + 1)
    return n


def _pad_order4(c, width):
    """An order-d coefficient table [..., n] as the order-4 table [..., width] of the same polynomials: zeros for the
    monomials of degree > d.  A fresh allocation (8-byte aligned, as the 126-wide backward kernels want it)."""
    return c if c.shape[-1] == width else torch.nn.functional.pad(c, (0, width - c.shape[-1]))


def _mask(mask, img):
    """-> (tensor or None, mask_kind).  Accepts None, bool/uint8 or floating [B|1,1,H,W].
    bool is what the reference passes (data.py:190: `mask > 0`).  A uint8 mask is read the same way -- NONZERO KEEPS the pixel --
    which equals torch's `img * mask` for bytes 0 / 1 only: a 0 / 255 mask straight from a PNG would scale by 255 in torch.
    A floating mask multiplies by its value, as torch does (pass `mask.float()` for that behaviour with other integer types)."""
    if mask is None:
        return None, MASK_NONE
    _need_device(mask, "mask")
    B, _, H, W = img.shape
    if mask.dim() == 3:
        mask = mask.unsqueeze(1)
    if mask.dim() != 4 or mask.shape[1] != 1 or mask.shape[2] != H or mask.shape[3] != W \
            or mask.shape[0] not in (1, B):
        raise ValueError(f"mask must be [B,1,H,W] matching img {tuple(img.shape)}, got {tuple(mask.shape)}")
    if mask.shape[0] != B:
        mask = mask.expand(B, 1, H, W)
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8), MASK_U8
    if mask.dtype == torch.uint8:
        return mask.contiguous(), MASK_U8
    if mask.is_floating_point():
        return mask.to(torch.float32).contiguous(), MASK_F32
    raise TypeError(f"mask dtype {mask.dtype} not supported (bool, uint8 or floating)")


def _workspace(B, n_knots, device):
    nbytes = _lib.load().curl_workspace_bytes(B, n_knots)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device), nbytes


def _ptr(t):
    return 0 if t is None else t.data_ptr()


# ------------------------------------------------------------------ curves.py
@_one_device
@_empty_ok(mask_arg=-1)
def apply_curve(img, C, slope_sqr_diff, channel_in, channel_out, flags=F_EXACT_ORDER):
    """curves.apply_curve (curves.py:4-38).  C are the knots after exp, [B,K].
    slope_sqr_diff [B] is updated in place (curves.py:24) and returned; None skips it.  Forward only."""
    if _grad_wanted(img, C, slope_sqr_diff):
        raise NotImplementedError("curl_amd: apply_curve has no backward; adjust_rgb / adjust_lab / adjust_hsv and the "
                                  "stages are differentiable. Use torch.no_grad() here.")
    lib = _lib.load()
    img = _image(img)
    B, _, H, W = img.shape
    Cc, K = _knots(C, "C", 1, B)
    reg = slope_sqr_diff
    if reg is not None:
        _need_device(reg, "slope_sqr_diff")
        if reg.shape != (B,) or reg.dtype != torch.float32 or not reg.is_contiguous():
            raise ValueError("slope_sqr_diff must be a contiguous float32 [B] tensor")
    out = torch.empty_like(img)
    rc = lib.curl_apply_curve_f32(img.data_ptr(), Cc.data_ptr(), out.data_ptr(), _ptr(reg), B, H, W, K,
                                  int(channel_in), int(channel_out), flags, _stream(img))
    _lib.check(rc, "curl_apply_curve_f32")
    return out, reg


def _adjust(fn_name, ncurves, img, raw, flags, return_workspace=False):  # noqa: E302
    lib = _lib.load()
    img = _image(img)
    B, _, H, W = img.shape
    rawc, K = _knots(raw, "knots", ncurves, B)
    out = torch.empty_like(img)
    reg = torch.empty(B, dtype=torch.float32, device=img.device)
    ws, nbytes = _workspace(B, rawc.shape[1], img.device)
    rc = getattr(lib, fn_name)(img.data_ptr(), rawc.data_ptr(), out.data_ptr(), reg.data_ptr(), ws.data_ptr(), nbytes,
                               B, H, W, K, flags, _stream(img))
    _lib.check(rc, fn_name)
    return (out, reg, ws) if return_workspace else (out, reg)


@_one_device
@_empty_ok(mask_arg=-1)
def _adjust_rgb(img, R, flags=0, return_workspace=False):
    return _adjust("curl_adjust_rgb_f32", 3, img, R, flags, return_workspace)


@_one_device
@_empty_ok(mask_arg=-1)
def _adjust_lab(img, L, flags=0, return_workspace=False):
    return _adjust("curl_adjust_lab_f32", 3, img, L, flags, return_workspace)


@_one_device
@_empty_ok(mask_arg=-1)
def _adjust_hsv(img, S, flags=0, return_workspace=False):
    return _adjust("curl_adjust_hsv_f32", 4, img, S, flags, return_workspace)


def adjust_rgb(img, R, flags=0):
    """curves.adjust_rgb (curves.py:90-133), regulariser seeded with zeros.  Differentiable (image and knots)."""
    if _grad_wanted(img, R):
        return _curve_op_grad("adjust_rgb", img, None, R, flags)
    return _adjust_rgb(img, R, flags)


def adjust_lab(img, L, flags=0):
    """curves.adjust_lab (curves.py:136-180).  Differentiable (image and knots)."""
    if _grad_wanted(img, L):
        return _curve_op_grad("adjust_lab", img, None, L, flags)
    return _adjust_lab(img, L, flags)


def adjust_hsv(img, S, flags=0):
    """curves.adjust_hsv (curves.py:41-87).  Differentiable (image and knots)."""
    if _grad_wanted(img, S):
        return _curve_op_grad("adjust_hsv", img, None, S, flags)
    return _adjust_hsv(img, S, flags)


# ------------------------------------------------------------------ colors.py
def _convert(fn_name, img, flags=0):
    lib = _lib.load()
    img = _image(img)
    B, _, H, W = img.shape
    out = torch.empty_like(img)
    rc = getattr(lib, fn_name)(img.data_ptr(), out.data_ptr(), B, H, W, flags, _stream(img))
    _lib.check(rc, fn_name)
    return out


@_one_device
@_empty_ok()
def _rgb2lab(img, flags=0):
    return _convert("curl_rgb2lab_f32", img, flags)


def rgb2lab(img, flags=0):
    """colors.RGB2LAB.forward (colors.py:27-62).  Differentiable."""
    if _grad_wanted(img):
        return _ConvertFn.apply("rgb2lab", img, flags)
    return _rgb2lab(img, flags)


@_one_device
@_empty_ok()
def _lab2rgb(img, flags=0):
    return _convert("curl_lab2rgb_f32", img, flags)


def lab2rgb(img, flags=0):
    """colors.LAB2RGB.forward (colors.py:88-123).  Differentiable."""
    if _grad_wanted(img):
        return _ConvertFn.apply("lab2rgb", img, flags)
    return _lab2rgb(img, flags)


@_one_device
@_empty_ok()
def _rgb2hsv(img, flags=0):
    return _convert("curl_rgb2hsv_f32", img, flags)


def rgb2hsv(img, flags=0):
    """colors.RGB2HSV.forward (colors.py:195-242).  Differentiable."""
    if _grad_wanted(img):
        return _ConvertFn.apply("rgb2hsv", img, flags)
    return _rgb2hsv(img, flags)


@_one_device
@_empty_ok()
def _hsv2rgb(img, flags=0):
    return _convert("curl_hsv2rgb_f32", img, flags)


def hsv2rgb(img, flags=0):
    """colors.HSV2RGB.forward (colors.py:131-177).  Differentiable."""
    if _grad_wanted(img):
        return _ConvertFn.apply("hsv2rgb", img, flags)
    return _hsv2rgb(img, flags)


# ------------------------------------------------------------------ model.py: fused stages
def lab_stage(img, mask, L, flags=0, out=None):
    """RGB -> Lab -> 3 curves -> *mask -> RGB in one pass (model.py:151-157). -> (rgb, reg_lab).
    Differentiable (image and knots; no mask gradient) in the default affine form."""
    if _grad_wanted(img, L):
        return _curve_op_grad("lab_stage", img, mask, L, flags, out)
    return _lab_stage(img, mask, L, flags=flags, out=out)


def _stage(fn_name, name, ncurves, img, mask, raw, flags, out, return_workspace):
    lib = _lib.load()
    img = _image(img)
    B, _, H, W = img.shape
    rawc, K = _knots(raw, name, ncurves, B)
    m, kind = _mask(mask, img)
    out = torch.empty_like(img) if out is None else _check_out(out, img)
    reg = torch.empty(B, dtype=torch.float32, device=img.device)
    ws, nbytes = _workspace(B, rawc.shape[1], img.device)
    rc = getattr(lib, fn_name)(img.data_ptr(), _ptr(m), kind, rawc.data_ptr(), out.data_ptr(), reg.data_ptr(),
                               ws.data_ptr(), nbytes, B, H, W, K, flags, _stream(img))
    _lib.check(rc, fn_name)
    return (out, reg, ws) if return_workspace else (out, reg)


@_one_device
@_empty_ok(mask_arg=0)
def _lab_stage(img, mask, L, flags=0, out=None, return_workspace=False):
    return _stage("curl_lab_stage_f32", "L", 3, img, mask, L, flags, out, return_workspace)


def hsv_stage(img, mask, H, flags=0, out=None):
    """RGB -> HSV -> 4 curves -> *mask -> RGB in one pass (model.py:163-169): the layer's RGB residual. -> (rgb, reg_hsv).
    Differentiable (image and knots; no mask gradient)."""
    if _grad_wanted(img, H):
        return _curve_op_grad("hsv_stage", img, mask, H, flags, out)
    return _hsv_stage(img, mask, H, flags=flags, out=out)


@_one_device
@_empty_ok(mask_arg=0)
def _hsv_stage(img, mask, H, flags=0, out=None, return_workspace=False):
    return _stage("curl_hsv_stage_f32", "H", 4, img, mask, H, flags, out, return_workspace)


def curl_layer_forward(img, mask, L, R, H, flags=0, out=None, return_workspace=False):
    """CURLLayer.forward (model.py:137-176) in one pass over the pixels. -> (img, reg[B]).
    L [B,3*Kl], R [B,3*Kr], H [B,4*Kh] are the already-sliced raw knots.
    return_workspace: also return the knot workspace the call filled (-> (img, reg, ws)); handed back to
    curl_layer_backward(..., workspace=ws) it saves that call its knot-prep launch.
    The plain call (every tensor on the current device, float32, contiguous, even knot counts) goes through the
    compiled binding (csrc/fastcall.cpp: one Python -> C++ transition); anything else -- and every error -- through the
    checked path below."""
    if type(img) is torch.Tensor:
        fast = _lib.fast()
        if fast is not None:
            r = fast.layer_fwd(img, mask, L, R, H, flags, out)
            if r is not None:
                if r.__class__ is int:
                    _lib.check(r, "curl_layer_fwd_f32")
                return r if return_workspace else r[:2]
    return _curl_layer_forward_checked(img, mask, L, R, H, flags=flags, out=out, return_workspace=return_workspace)


@_one_device
@_empty_ok(mask_arg=0)
def _curl_layer_forward_checked(img, mask, L, R, H, flags=0, out=None, return_workspace=False):
    lib = _lib.load()
    img = _image(img)
    B, _, Hh, W = img.shape
    Lc, Rc, Hc, Kl, Kr, Kh, n_knots = _layer_knots(L, R, H, B)
    m, kind = _mask(mask, img)
    out = torch.empty_like(img) if out is None else _check_out(out, img)
    reg = torch.empty(B, dtype=torch.float32, device=img.device)
    ws, nbytes = _workspace(B, n_knots, img.device)
    rc = lib.curl_layer_fwd_f32(img.data_ptr(), _ptr(m), kind, Lc.data_ptr(), Rc.data_ptr(), Hc.data_ptr(),
                                out.data_ptr(), reg.data_ptr(), ws.data_ptr(), nbytes, B, Hh, W, Kl, Kr, Kh,
                                flags, _stream(img))
    _lib.check(rc, "curl_layer_fwd_f32")
    return (out, reg, ws) if return_workspace else (out, reg)


def _slab(rows, H):
    r0, r1 = int(rows[0]), int(rows[1])
    if not (0 <= r0 < r1 <= H):
        raise ValueError(f"rows must satisfy 0 <= r0 < r1 <= H={H}, got {rows}")
    return r0, r1 - r0


@_one_device
def curl_layer_forward_rows(img, mask, L, R, H, rows, out, flags=0):
    """CURLLayer.forward on rows [r0, r1) of every image of the FULL tensors, in place in `out` (full-size, required):
    the split-pixels layout (shard.apply_row_slab) without the .contiguous() copy of a row slice.  Rows outside the
    slab are neither read nor written.  -> (out, reg[B])."""
    lib = _lib.load()
    img = _image(img)
    B, _, Hh, W = img.shape
    r0, n = _slab(rows, Hh)
    Lc, Rc, Hc, Kl, Kr, Kh, n_knots = _layer_knots(L, R, H, B)
    m, kind = _mask(mask, img)
    out = _check_out(out, img)
    reg = torch.empty(B, dtype=torch.float32, device=img.device)
    ws, nbytes = _workspace(B, n_knots, img.device)
    rc = lib.curl_layer_fwd_slab_f32(img.data_ptr(), _ptr(m), kind, Lc.data_ptr(), Rc.data_ptr(), Hc.data_ptr(),
                                     out.data_ptr(), reg.data_ptr(), ws.data_ptr(), nbytes, B, Hh, W, r0, n, Kl, Kr, Kh,
                                     flags, _stream(img))
    _lib.check(rc, "curl_layer_fwd_slab_f32")
    return out, reg


@_one_device
def trispace_forward_rows(img, coeffs, rows, out, residual_only=False):
    """trispace_forward on rows [r0, r1) of every image of the FULL tensors (pixel coordinates stay the full image's:
    the rows written equal the same rows of the whole-image call bit for bit)."""
    lib = _lib.load()
    img = _image(img)
    B, _, H, W = img.shape
    r0, n = _slab(rows, H)
    _check_coeffs(coeffs, B)
    c = _coeffs32(coeffs, pairs=coeffs.shape[3] == 126)
    out = _check_out(out, img)
    rc = lib.curl_trispace_fwd_slab_f32(img.data_ptr(), c.data_ptr(), out.data_ptr(), B, H, W, r0, n, _nc_arg(c.shape[3]),
                                        _lib.F_RESIDUAL_ONLY if residual_only else 0, _stream(img))
    _lib.check(rc, "curl_trispace_fwd_slab_f32")
    return out


def _image_and_grad(img, grad_out):
    """A backward's image and the gradient at its output: both [B,3,H,W] float32, the same shape."""
    img = _image(img)
    grad_out = _image(grad_out, "grad_out")
    if grad_out.shape != img.shape:
        raise ValueError(f"grad_out {tuple(grad_out.shape)} does not match img {tuple(img.shape)}")
    return img, grad_out


def _grad_reg32(grad_reg, B):
    if grad_reg is None:
        return None
    _need_device(grad_reg, "grad_reg")
    grad_reg = grad_reg.to(torch.float32).contiguous()
    if grad_reg.shape != (B,):
        raise ValueError("grad_reg must be [B]")
    return grad_reg


def _bwd_setup(lib, img, grad_reg, n_knots, workspace, flags, ws_source, sbytes=None):
    """What the layer and the curve backwards share: grad_reg as float32 [B] (or None), the knot workspace -- the caller's
    (CURL_F_WS_READY: `ws_source` filled it for the same knots, the entry point skips its knot prep) or a fresh one -- and
    the block-partials scratch (sbytes: its size, curl_layer_bwd_scratch_bytes by default).
    -> (grad_reg, ws, nbytes, bflags, scratch, sbytes)"""
    B, _, H, W = img.shape
    grad_reg = _grad_reg32(grad_reg, B)
    ws, nbytes = _workspace(B, n_knots, img.device)
    bflags = flags & F_MASK_FIRST  # the one forward flag that means something here
    if workspace is not None:
        if workspace.device != img.device or workspace.dtype != torch.float32 or workspace.numel() * 4 < nbytes:
            raise ValueError(f"workspace is not the tensor {ws_source} for this batch")
        ws, bflags = workspace, bflags | _lib.F_WS_READY
    if sbytes is None:
        sbytes = lib.curl_layer_bwd_scratch_bytes(B, H, W)
    scratch = torch.empty(sbytes // 4, dtype=torch.float32, device=img.device)
    return grad_reg, ws, nbytes, bflags, scratch, sbytes


def curl_layer_backward(img, mask, L, R, H, grad_out, grad_reg=None, need_grad_img=True, workspace=None, flags=0):
    """Backward of curl_layer_forward (what autograd would run through model.py:137-176).
    -> (grad_img or None, grad_L, grad_R, grad_H).
    workspace: the tensor curl_layer_forward(..., return_workspace=True) returned for the SAME knots (CURL_F_WS_READY).
    flags: F_MASK_FIRST (bool / uint8 foreground masks); F_PWL: the backward of curl_layer_forward(..., flags=F_PWL), the
    paper's piecewise-linear curves (curl_layer_pwl_bwd_f32; even knot splits only).
    (Plain affine calls through the compiled binding, as curl_layer_forward.)"""
    if flags & F_PWL:  # (before the binding, which knows the affine entry point only)
        return _curl_layer_backward_checked(img, mask, L, R, H, grad_out, grad_reg=grad_reg, need_grad_img=need_grad_img,
                                            workspace=workspace, flags=flags)
    fast = _lib.fast() if type(img) is torch.Tensor else None
    if fast is not None:
        r = fast.layer_bwd(img, mask, L, R, H, grad_out, grad_reg, need_grad_img, workspace, flags & F_MASK_FIRST)
        if r is not None:
            if r.__class__ is int:
                _lib.check(r, "curl_layer_bwd_f32")
            return r
    return _curl_layer_backward_checked(img, mask, L, R, H, grad_out, grad_reg=grad_reg, need_grad_img=need_grad_img,
                                        workspace=workspace, flags=flags)


@_one_device
def _curl_layer_backward_checked(img, mask, L, R, H, grad_out, grad_reg=None, need_grad_img=True, workspace=None, flags=0):
    lib = _lib.load()
    pwl = bool(flags & F_PWL)
    if pwl and _is_empty_image(img):
        # an empty image owes only the regulariser's share: the same entry point on a 1x1 stand-in with a zero gradient
        _need_device(img, "img")
        B = img.shape[0]
        g_img = torch.empty_like(img) if need_grad_img else None
        if B == 0:
            return (g_img,) + tuple(torch.zeros(t.shape, dtype=torch.float32, device=img.device) for t in (L, R, H))
        z = img.new_zeros((B, 3, 1, 1))
        return (g_img,) + _curl_layer_backward_checked(z, None, L, R, H, z, grad_reg, False, None, flags)[1:]
    img, grad_out = _image_and_grad(img, grad_out)
    B, _, Hh, W = img.shape
    Lc, Rc, Hc, Kl, Kr, Kh, n_knots = _layer_knots(L, R, H, B)
    m, kind = _mask(mask, img)
    g_img = torch.empty_like(img) if need_grad_img else None
    gL, gR, gH = torch.empty_like(Lc), torch.empty_like(Rc), torch.empty_like(Hc)
    grad_reg, ws, nbytes, bflags, scratch, sbytes = _bwd_setup(
        lib, img, grad_reg, n_knots, workspace, flags, "curl_layer_forward returned",
        lib.curl_layer_pwl_bwd_scratch_bytes(B, Hh, W, Kl, Kr, Kh) if pwl else None)
    name = "curl_layer_pwl_bwd_f32" if pwl else "curl_layer_bwd_f32"
    rc = getattr(lib, name)(img.data_ptr(), _ptr(m), kind, Lc.data_ptr(), Rc.data_ptr(), Hc.data_ptr(),
                            grad_out.data_ptr(), _ptr(grad_reg), _ptr(g_img), gL.data_ptr(), gR.data_ptr(),
                            gH.data_ptr(), ws.data_ptr(), nbytes, scratch.data_ptr(), sbytes, B, Hh, W, Kl, Kr, Kh,
                            bflags, _stream(img))
    _lib.check(rc, name)
    return g_img, gL, gR, gH


# ------------------------------------------------------------------ backward of the stand-alone curve ops and stages
# op -> (C entry point, curves, forward, takes a mask)
_CURVE_BWD = {
    "adjust_rgb": ("curl_adjust_rgb_bwd_f32", 3, "_adjust_rgb", False),
    "adjust_lab": ("curl_adjust_lab_bwd_f32", 3, "_adjust_lab", False),
    "adjust_hsv": ("curl_adjust_hsv_bwd_f32", 4, "_adjust_hsv", False),
    "lab_stage": ("curl_lab_stage_bwd_f32", 3, "_lab_stage", True),
    "hsv_stage": ("curl_hsv_stage_bwd_f32", 4, "_hsv_stage", True),
}


@_one_device
def _curve_backward(op, img, mask, raw, grad_out, grad_reg=None, need_grad_img=True, workspace=None, flags=0):
    """-> (grad_img or None, grad_raw): the backward of one stand-alone curve op or stage (_CURVE_BWD)."""
    fn_name, ncurves, _, masked = _CURVE_BWD[op]
    lib = _lib.load()
    if _is_empty_image(img):
        # an empty image owes only the regulariser's share: the same entry point on a 1x1 stand-in with a zero gradient
        _need_device(img, "img")
        B = img.shape[0]
        g_img = torch.empty_like(img) if need_grad_img else None
        if B == 0:
            return g_img, torch.zeros(raw.shape, dtype=torch.float32, device=img.device)
        z = img.new_zeros((B, 3, 1, 1))
        _, g_raw = _curve_backward(op, z, None, raw, z, grad_reg, False, None, flags)
        return g_img, g_raw
    img, grad_out = _image_and_grad(img, grad_out)
    B, _, Hh, W = img.shape
    rawc, K = _knots(raw, "knots", ncurves, B)
    g_img = torch.empty_like(img) if need_grad_img else None
    g_raw = torch.empty_like(rawc)
    grad_reg, ws, nbytes, bflags, scratch, sbytes = _bwd_setup(lib, img, grad_reg, rawc.shape[1], workspace, flags,
                                                               f"ops.{op} filled")
    head = (img.data_ptr(),)
    if masked:
        m, kind = _mask(mask, img)
        head = (img.data_ptr(), _ptr(m), kind)
    rc = getattr(lib, fn_name)(*head, rawc.data_ptr(), grad_out.data_ptr(), _ptr(grad_reg), _ptr(g_img), g_raw.data_ptr(),
                               ws.data_ptr(), nbytes, scratch.data_ptr(), sbytes, B, Hh, W, K, bflags, _stream(img))
    _lib.check(rc, fn_name)
    return g_img, g_raw


def adjust_rgb_backward(img, R, grad_out, grad_reg=None, need_grad_img=True, workspace=None):
    """Backward of adjust_rgb (torch autograd through curves.py:90-133). -> (grad_img or None, grad_R).
    workspace: the one adjust_rgb filled for the SAME knots (CURL_F_WS_READY: no knot-prep launch)."""
    return _curve_backward("adjust_rgb", img, None, R, grad_out, grad_reg, need_grad_img, workspace)


def adjust_lab_backward(img, L, grad_out, grad_reg=None, need_grad_img=True, workspace=None):
    """Backward of adjust_lab (curves.py:136-180). -> (grad_img or None, grad_L)."""
    return _curve_backward("adjust_lab", img, None, L, grad_out, grad_reg, need_grad_img, workspace)


def adjust_hsv_backward(img, S, grad_out, grad_reg=None, need_grad_img=True, workspace=None):
    """Backward of adjust_hsv (curves.py:41-87). -> (grad_img or None, grad_S)."""
    return _curve_backward("adjust_hsv", img, None, S, grad_out, grad_reg, need_grad_img, workspace)


def lab_stage_backward(img, mask, L, grad_out, grad_reg=None, need_grad_img=True, workspace=None, flags=0):
    """Backward of lab_stage (model.py:151-157). -> (grad_img or None, grad_L); no mask gradient.
    flags: F_MASK_FIRST is honoured (bool / uint8 foreground masks), nothing else."""
    return _curve_backward("lab_stage", img, mask, L, grad_out, grad_reg, need_grad_img, workspace, flags)


def hsv_stage_backward(img, mask, H, grad_out, grad_reg=None, need_grad_img=True, workspace=None, flags=0):
    """Backward of hsv_stage (model.py:163-169). -> (grad_img or None, grad_H); no mask gradient."""
    return _curve_backward("hsv_stage", img, mask, H, grad_out, grad_reg, need_grad_img, workspace, flags)


@_one_device
def _convert_backward(name, img, grad_out):
    if _is_empty_image(img):
        _need_device(img, "img")
        return torch.empty_like(img)
    lib = _lib.load()
    img, grad_out = _image_and_grad(img, grad_out)
    B, _, H, W = img.shape
    g = torch.empty_like(img)
    fn_name = f"curl_{name}_bwd_f32"
    rc = getattr(lib, fn_name)(img.data_ptr(), grad_out.data_ptr(), g.data_ptr(), B, H, W, 0, _stream(img))
    _lib.check(rc, fn_name)
    return g


def rgb2lab_backward(img, grad_out):
    """Backward of rgb2lab (autograd through colors.py:27-62) at the input img. -> grad_img."""
    return _convert_backward("rgb2lab", img, grad_out)


def lab2rgb_backward(img, grad_out):
    """Backward of lab2rgb (colors.py:88-123). -> grad_img."""
    return _convert_backward("lab2rgb", img, grad_out)


def rgb2hsv_backward(img, grad_out):
    """Backward of rgb2hsv (colors.py:195-242). -> grad_img."""
    return _convert_backward("rgb2hsv", img, grad_out)


def hsv2rgb_backward(img, grad_out):
    """Backward of hsv2rgb (colors.py:131-177). -> grad_img."""
    return _convert_backward("hsv2rgb", img, grad_out)


def _grad_wanted(*tensors):
    """The test CURLLayer.forward uses: an autograd node only when grad mode is on and some tensor input requires grad."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


class _CurveOpFn(torch.autograd.Function):
    """Autograd node of a stand-alone curve op or stage (_CURVE_BWD), as model._CurlLayerFn: the forward is the no-grad
    call (the same launches, the same bits), its knot workspace rides along to the backward."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, op, img, mask, raw, flags, out):
        fwd = globals()[_CURVE_BWD[op][2]]
        if _CURVE_BWD[op][3]:
            o, reg, ws = fwd(img, mask, raw, flags=flags, out=out, return_workspace=True)
        else:
            o, reg, ws = fwd(img, raw, flags=flags, return_workspace=True)
        ctx.save_for_backward(img, raw, ws)
        ctx.op, ctx.mask, ctx.flags = op, mask, flags
        return o, reg

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out, grad_reg):
        img, raw, ws = ctx.saved_tensors
        g_img, g_raw = _curve_backward(ctx.op, img, ctx.mask, raw, grad_out.contiguous(), grad_reg, ctx.needs_input_grad[1],
                                       workspace=ws, flags=ctx.flags)
        return None, g_img, None, g_raw.to(raw.dtype) if ctx.needs_input_grad[3] else None, None, None


def _curve_op_grad(op, img, mask, raw, flags, out=None):
    if flags & F_PWL:
        raise NotImplementedError(f"curl_amd: {op} with F_PWL (the paper's piecewise-linear curves) has no backward; "
                                  "use torch.no_grad() or the default affine form")
    return _CurveOpFn.apply(op, img, mask, raw, flags, out)


class _ConvertFn(torch.autograd.Function):
    """Autograd node of a stand-alone colour converter: forward = the no-grad call, backward = curl_<name>_bwd_f32."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, name, img, flags):
        ctx.save_for_backward(img)
        ctx.name = name
        return globals()["_" + name](img, flags)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        (img,) = ctx.saved_tensors
        return None, _convert_backward(ctx.name, img, grad_out.contiguous()), None


# ------------------------------------------------------------------ polynomial path (model.py:206-520)
@_one_device
@_empty_ok()
def trispace_forward(img, coeffs, residual_only=False, flags=0):
    """TriSpaceRegNet.generate_residual (+ generate_image unless residual_only), model.py:499-520, in one pass.
    coeffs [B,3,3,NC] with NC = 126 (spatial) or 35 for polynomial order 4, 56|20, 21|10, 6|4 for orders 3, 2, 1: each
    order runs a kernel of its own; [:,0]=R, [:,1]=L, [:,2]=H (model.py:526)."""
    lib = _lib.load()
    img = _image(img)
    B, _, H, W = img.shape
    _check_coeffs(coeffs, B)
    c = _coeffs32(coeffs, pairs=coeffs.shape[3] == 126)
    out = torch.empty_like(img)
    rc = lib.curl_trispace_fwd_f32(img.data_ptr(), c.data_ptr(), out.data_ptr(), B, H, W, _nc_arg(c.shape[3]),
                                   flags | (_lib.F_RESIDUAL_ONLY if residual_only else 0), _stream(img))
    _lib.check(rc, "curl_trispace_fwd_f32")
    return out


@_one_device
def trispace_backward(img, coeffs, grad_out, residual_only=False):
    """d loss / d coeffs [B,3,3,NC] of trispace_forward, given grad_out = d loss / d out."""
    lib = _lib.load()
    img, grad_out = _image(img), _image(grad_out, "grad_out")
    B, _, H, W = img.shape
    _check_coeffs(coeffs, B)
    n = coeffs.shape[3]
    nc = _ORDER4_WIDTH[n]  # orders 1-3 run the order-4 kernels on the zero-padded table (_pad_order4)
    c = _pad_order4(_coeffs32(coeffs, pairs=n == 126), nc)
    g = torch.empty_like(c)
    nbytes = lib.curl_trispace_bwd_scratch_bytes(B, H, W, nc)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=img.device)
    rc = lib.curl_trispace_bwd_f32(img.data_ptr(), c.data_ptr(), grad_out.data_ptr(), g.data_ptr(), scratch.data_ptr(),
                                   nbytes, B, H, W, nc, _lib.F_RESIDUAL_ONLY if residual_only else 0, _stream(img))
    _lib.check(rc, "curl_trispace_bwd_f32")
    return g if n == nc else g[..., :n].contiguous()


TRISPACE_IMG_GRAD_TILE = 4096  # pixels per workgroup of trispace_backward_img's float4 kernel (256 lanes x 4 pixels x 4 steps)


@_one_device
@_empty_ok()
def trispace_backward_img(img, coeffs, grad_out, residual_only=False):
    """d loss / d img [B,3,H,W] of trispace_forward, given grad_out = d loss / d out (include/curl_hip_grad.h): one per-pixel
    pass, no scratch.  The coordinates of the spatial form are data."""
    lib = _lib.load()
    img, grad_out = _image(img), _image(grad_out, "grad_out")
    B, _, H, W = img.shape
    if grad_out.shape != img.shape:
        raise ValueError(f"grad_out must have img's shape {tuple(img.shape)}, got {tuple(grad_out.shape)}")
    _check_coeffs(coeffs, B)
    n = coeffs.shape[3]
    c = _pad_order4(_coeffs32(coeffs, pairs=n == 126), _ORDER4_WIDTH[n])  # orders 1-3: the order-4 kernel, as trispace_backward
    g = torch.empty_like(img)
    rc = lib.curl_trispace_bwd_img_f32(img.data_ptr(), c.data_ptr(), grad_out.data_ptr(), g.data_ptr(), B, H, W, c.shape[3],
                                       _lib.F_RESIDUAL_ONLY if residual_only else 0, _stream(img))
    _lib.check(rc, "curl_trispace_bwd_img_f32")
    return g


def _poly_layer_args(img, coeffs):
    """The stand-alone polynomial layer's tensor checks: img float32 [B,3|5,H,W], coeffs [B,3,n] with n the coefficient count
    of degree 1..4 in that many variables -> (img, coeffs, degree)."""
    _need_device(img, "img")
    _need_device(coeffs, "coeffs")
    if img.dim() != 4 or img.shape[1] not in (3, 5) or img.dtype != torch.float32:
        raise ValueError(f"img must be float32 [B,3|5,H,W], got {tuple(img.shape)} {img.dtype}")
    B, V, H, W = img.shape
    counts = POLY_COEFFS[V]
    if coeffs.dim() != 3 or tuple(coeffs.shape[:2]) != (B, 3) or coeffs.shape[2] not in counts:
        raise ValueError(f"coeffs must be [B={B},3,{counts[3]}], got {tuple(coeffs.shape)} "
                         f"(degrees 3, 2, 1: {counts[2]}, {counts[1]}, {counts[0]} in place of {counts[3]})")
    return img.contiguous(), _coeffs32(coeffs, pairs=False), counts.index(coeffs.shape[2]) + 1  # the kernels read scalars


@_one_device
def poly_layer(img, coeffs):
    """ChannelPolyLayer(degree) / Deg4MobilePolyLayer forward (model.py:295-333, 399-415):
    img [B,V,H,W] with V = 5 or 3, coeffs [B,3,n] -> [B,3,H,W]; n = 126|35 for degree 4, 56|20, 21|10, 6|4 for degrees 3, 2, 1
    (the width names the degree; each has a kernel of its own)."""
    lib = _lib.load()
    img, c, degree = _poly_layer_args(img, coeffs)
    B, V, H, W = img.shape
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=img.device)
    _lib.check(lib.curl_poly_layer_f32(img.data_ptr(), c.data_ptr(), out.data_ptr(), B, H, W, _lib.poly_vars(V, degree),
                                       _stream(img)), "curl_poly_layer_f32")
    return out


def poly_layer_bwd_tile(B, H, W):
    """Pixels per tile of poly_layer_backward's coefficient-gradient pass (include/curl_hip.h: 1024 * steps)."""
    return 1024 * min(max(B * H * W >> 20, 4), 16)


@_one_device
def poly_layer_backward(img, coeffs, grad_out, need_img_grad=True, need_coeffs_grad=True):
    """Backward of poly_layer: grad_out [B,3,H,W] = d loss / d out -> (grad_img [B,V,H,W] | None, grad_coeffs [B,3,n] |
    None).  A gradient that is not needed is neither computed nor stored (its kernels are not launched).  Degrees 1-3 run the
    degree-4 kernels on the zero-padded table (_pad_order4); their coefficient gradient is cut back to n."""
    lib = _lib.load()
    img, c, _ = _poly_layer_args(img, coeffs)
    B, V, H, W = img.shape
    n = c.shape[2]
    c = _pad_order4(c, POLY_COEFFS[V][3])
    _need_device(grad_out, "grad_out")
    if tuple(grad_out.shape) != (B, 3, H, W) or grad_out.dtype != torch.float32:
        raise ValueError(f"grad_out must be float32 [B={B},3,{H},{W}], got {tuple(grad_out.shape)} {grad_out.dtype}")
    if not need_img_grad and not need_coeffs_grad:
        return None, None
    grad_out = grad_out.contiguous()
    g_img = torch.empty_like(img) if need_img_grad else None
    g_c = torch.empty_like(c) if need_coeffs_grad else None
    nbytes = lib.curl_poly_layer_bwd_scratch_bytes(B, H, W, V) if need_coeffs_grad else 0
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=img.device) if need_coeffs_grad else None
    rc = lib.curl_poly_layer_bwd_f32(img.data_ptr(), c.data_ptr(), grad_out.data_ptr(), _ptr(g_img), _ptr(g_c), _ptr(scratch),
                                     nbytes, B, H, W, V, 0, _stream(img))
    _lib.check(rc, "curl_poly_layer_bwd_f32")
    return g_img, (g_c if g_c is None or g_c.shape[2] == n else g_c[..., :n].contiguous())


# ------------------------------------------------------------------ layout edges
@_one_device
def u8hwc_to_f32chw(x):
    """uint8 [B,H,W,3|4] (or [H,W,C]) -> float32 [B,3,H,W] = value/255 (infer.py:35-40, transpose.py:19-31)."""
    lib = _lib.load()
    _need_device(x, "x")
    if x.dtype != torch.uint8:
        raise TypeError(f"expected uint8, got {x.dtype}")
    squeeze = x.dim() == 3
    if squeeze:
        x = x.unsqueeze(0)
    if x.dim() != 4 or x.shape[3] not in (3, 4):
        raise ValueError(f"expected [B,H,W,3|4], got {tuple(x.shape)}")
    x = x.contiguous()
    B, H, W, C = x.shape
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=x.device)
    _lib.check(lib.curl_u8hwc_to_f32chw(x.data_ptr(), out.data_ptr(), B, H, W, C, _stream(x)), "curl_u8hwc_to_f32chw")
    return out[0] if squeeze else out


@_one_device
def f32chw_to_u8hwc(x):
    """float32 [B,3,H,W] (or [3,H,W]) -> uint8 [B,H,W,3], (x*255) TRUNCATED (evaluate.py:64-66)."""
    lib = _lib.load()
    squeeze = isinstance(x, torch.Tensor) and x.dim() == 3
    if squeeze:
        x = x.unsqueeze(0)
    x = _image(x, "x")
    B, _, H, W = x.shape
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=x.device)
    _lib.check(lib.curl_f32chw_to_u8hwc(x.data_ptr(), out.data_ptr(), B, H, W, _stream(x)), "curl_f32chw_to_u8hwc")
    return out[0] if squeeze else out


@_one_device
def compose_white_u8hwc(x, mask):
    """infer.py:46-47 in one pass: x*mask + (1-mask), then (.*255) truncated to uint8, CHW -> HWC."""
    lib = _lib.load()
    squeeze = isinstance(x, torch.Tensor) and x.dim() == 3
    if squeeze:
        x = x.unsqueeze(0)
        mask = mask.unsqueeze(0) if mask.dim() == 3 else mask
    x = _image(x, "x")
    m, kind = _mask(mask, x)
    if m is None:
        raise ValueError("compose_white_u8hwc needs a mask")
    B, _, H, W = x.shape
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=x.device)
    _lib.check(lib.curl_compose_white_u8hwc(x.data_ptr(), m.data_ptr(), kind, out.data_ptr(), B, H, W, _stream(x)),
               "curl_compose_white_u8hwc")
    return out[0] if squeeze else out


def _bytes_image(x, name="img"):
    _need_device(x, name)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
        raise ValueError(f"{name} must be uint8 [B,H,W,3] (PIL's RGB layout), got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def _white(white_mask, img_u8):
    if white_mask is None:
        return None
    _need_device(white_mask, "white_mask")
    B, H, W, _ = img_u8.shape
    if white_mask.dtype != torch.uint8 or tuple(white_mask.shape) != (B, H, W):
        raise ValueError(f"white_mask must be uint8 [B,H,W] ('L' image), got {white_mask.dtype} {tuple(white_mask.shape)}")
    return white_mask.contiguous()


def trispace_forward_u8hwc(img_u8, coeffs, white_mask=None):
    """infer.py:35-47 on the file's own bytes, one launch: byte/255 -> generate_residual + generate_image ->
    [out*m + (1-m), m = white_mask/255] -> truncating *255.  img_u8 [B,H,W,3] uint8 -> [B,H,W,3] uint8.
    (Plain calls through the compiled binding, as curl_layer_forward.)"""
    fast = _lib.fast() if type(img_u8) is torch.Tensor else None
    if fast is not None:
        r = fast.trispace_fwd_u8hwc(img_u8, coeffs, white_mask)
        if r is not None:
            if r.__class__ is int:
                _lib.check(r, "curl_trispace_fwd_u8hwc")
            return r
    return _trispace_forward_u8hwc_checked(img_u8, coeffs, white_mask=white_mask)


@_one_device
def _trispace_forward_u8hwc_checked(img_u8, coeffs, white_mask=None):
    lib = _lib.load()
    x = _bytes_image(img_u8)
    B, H, W, _ = x.shape
    _check_coeffs(coeffs, B)
    c = _coeffs32(coeffs, pairs=coeffs.shape[3] == 126)
    wm = _white(white_mask, x)
    out = torch.empty_like(x)
    rc = lib.curl_trispace_fwd_u8hwc(x.data_ptr(), c.data_ptr(), _ptr(wm), out.data_ptr(), B, H, W, _nc_arg(c.shape[3]), 0,
                                     _stream(x))
    _lib.check(rc, "curl_trispace_fwd_u8hwc")
    return out


@_one_device
def curl_layer_forward_u8hwc(img_u8, mask, L, R, H, white_mask=None):
    """CURLLayer.forward between byte images: byte/255 -> the layer (mask [B,1,H,W] as in curl_layer_forward) ->
    [white background] -> truncating *255.  -> (uint8 [B,H,W,3], reg [B])."""
    lib = _lib.load()
    x = _bytes_image(img_u8)
    B, Hh, W, _ = x.shape
    Lc, Rc, Hc, Kl, Kr, Kh, n_knots = _layer_knots(L, R, H, B)
    m, kind = _mask(mask, SimpleNamespace(shape=(B, 3, Hh, W)))
    wm = _white(white_mask, x)
    out = torch.empty_like(x)
    reg = torch.empty(B, dtype=torch.float32, device=x.device)
    ws, nbytes = _workspace(B, n_knots, x.device)
    rc = lib.curl_layer_fwd_u8hwc(x.data_ptr(), _ptr(m), kind, Lc.data_ptr(), Rc.data_ptr(), Hc.data_ptr(), _ptr(wm),
                                  out.data_ptr(), reg.data_ptr(), ws.data_ptr(), nbytes, B, Hh, W, Kl, Kr, Kh, 0,
                                  _stream(x))
    _lib.check(rc, "curl_layer_fwd_u8hwc")
    return out, reg


def _bytes_image_fg(x, fg_mask):
    """The foreground entries' image and mask: uint8 [B,H,W,3|4] (alpha is not read) and uint8 [B,H,W], required."""
    _need_device(x, "img_u8")
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] not in (3, 4):
        raise ValueError(f"img_u8 must be uint8 [B,H,W,3|4] (PIL's RGB / RGBA layout), got {x.dtype} {tuple(x.shape)}")
    if x.numel() == 0:
        raise ValueError(f"img_u8 is empty: {tuple(x.shape)}")
    if fg_mask is None:
        raise ValueError("fg_mask is required (uint8 [B,H,W], the 'L' mask)")
    _need_device(fg_mask, "fg_mask")
    if fg_mask.dtype != torch.uint8 or tuple(fg_mask.shape) != tuple(x.shape[:3]):
        raise ValueError(f"fg_mask must be uint8 [B,H,W] ('L' image), got {fg_mask.dtype} {tuple(fg_mask.shape)}")
    return x.contiguous(), fg_mask.contiguous()


@_one_device
def trispace_foreground_u8hwc(img_u8, coeffs, fg_mask):
    """trispace_forward_u8hwc with white_mask = fg_mask for a segmentation mask, byte for byte the same result: wavefronts
    whose mask bytes are all 0 store white and never read their pixels (curl_trispace_fwd_fg_u8hwc).
    img_u8 uint8 [B,H,W,3|4] (alpha is not read), fg_mask uint8 [B,H,W] -> uint8 [B,H,W,3]."""
    lib = _lib.load()
    x, fg = _bytes_image_fg(img_u8, fg_mask)
    B, H, W, C = x.shape
    _check_coeffs(coeffs, B)
    c = _coeffs32(coeffs, pairs=coeffs.shape[3] == 126)
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=x.device)
    rc = lib.curl_trispace_fwd_fg_u8hwc(x.data_ptr(), C, c.data_ptr(), fg.data_ptr(), out.data_ptr(), B, H, W,
                                        _nc_arg(c.shape[3]), 0, _stream(x))
    _lib.check(rc, "curl_trispace_fwd_fg_u8hwc")
    return out


@_one_device
def curl_layer_foreground_u8hwc(img_u8, L, R, H, fg_mask):
    """curl_layer_forward_u8hwc(img, None, L, R, H, white_mask=fg_mask) for a segmentation mask, byte for byte the same result
    and the same reg (curl_layer_fwd_fg_u8hwc).  img_u8 uint8 [B,H,W,3|4] -> (uint8 [B,H,W,3], reg [B])."""
    lib = _lib.load()
    x, fg = _bytes_image_fg(img_u8, fg_mask)
    B, Hh, W, C = x.shape
    Lc, Rc, Hc, Kl, Kr, Kh, n_knots = _layer_knots(L, R, H, B)
    out = torch.empty(B, Hh, W, 3, dtype=torch.uint8, device=x.device)
    reg = torch.empty(B, dtype=torch.float32, device=x.device)
    ws, nbytes = _workspace(B, n_knots, x.device)
    rc = lib.curl_layer_fwd_fg_u8hwc(x.data_ptr(), C, Lc.data_ptr(), Rc.data_ptr(), Hc.data_ptr(), fg.data_ptr(), out.data_ptr(),
                                     reg.data_ptr(), ws.data_ptr(), nbytes, B, Hh, W, Kl, Kr, Kh, 0, _stream(x))
    _lib.check(rc, "curl_layer_fwd_fg_u8hwc")
    return out, reg


# ------------------------------------------------------------------ ragged batches (include/curl_hip_ragged.h)
_ragged_plans = {}  # (shapes, channels, has_mask, operator, device) -> _RaggedPlan
_RAGGED_PLANS_KEPT = 16


class _RaggedPlan:
    """One plan of the library's: the host copy (int32), its upload (None for a host-only plan) and what the callers read from
    it -- the arena sizes and the per-image offsets, from the descriptors as the header documents them."""

    def __init__(self, host, dev):
        self.host, self.dev = host, dev
        w = host.numpy()
        hw, dw = _lib.RAGGED_HEADER_WORDS, _lib.RAGGED_DESC_WORDS
        B = int(w[1])
        self.nbytes = host.numel() * 4
        self.img_bytes, self.mask_bytes, self.out_bytes = (int(v) for v in w[12:18].view("int64"))
        d = w[hw:hw + B * dw].reshape(B, dw)
        off = d[:, 10:16].copy().view("int64")  # img_off, mask_off, out_off per descriptor
        order = d[:, 1].argsort()               # the descriptors are sorted by class: back to image order
        self.img_off, self.mask_off, self.out_off = ([int(v) for v in off[order, k]] for k in range(3))


def _cached_plan(cache, kept, key, build):
    """cache[key]; a plan that is not there yet is built (build(): on the host by the library, then uploaded) and kept, the
    oldest of `kept` plans dropped for it."""
    plan = cache.get(key)
    if plan is None:
        plan = build()
        if len(cache) >= kept:
            del cache[next(iter(cache))]
        cache[key] = plan
    return plan


def _host_plan(builder, shapes, channels, max_images, tail, size_args=lambda hs, ws: ()):
    """The host copy (int32) of the plan the library's `builder` makes of a shape list: builder(B, H, W[, channels], *tail,
    buffer, bytes), the buffer sized by builder + "_bytes" (B, *size_args(H, W))."""
    import numpy as np
    lib = _lib.load()
    B = len(shapes)
    if B > max_images:
        raise ValueError(f"a ragged batch holds at most {max_images} images, got {B}")
    dims = [[s[0] for s in shapes], [s[1] for s in shapes]] + ([channels] if channels is not None else [])
    dims = [np.ascontiguousarray(v, dtype=np.int32) for v in dims]
    ptrs = [d.ctypes.data for d in dims]
    nbytes = getattr(lib, builder + "_bytes")(B, *size_args(*ptrs[:2]))
    host = torch.zeros(max(nbytes, 8) // 4, dtype=torch.int32)
    _lib.check(getattr(lib, builder)(B, *ptrs, *tail, host.data_ptr(), nbytes), builder)
    return host


def _ragged_plan(shapes, channels, has_mask, nc_arg, device):
    """The plan of a shape list for one operator (nc_arg: the entries' num_coeffs, 0 = the curve layer), built on the host by
    the library, uploaded once and kept (device None: host only); the oldest of more than sixteen is dropped."""
    def build():
        host = _host_plan("curl_ragged_plan", shapes, channels, _lib.RAGGED_MAX_IMAGES, (int(bool(has_mask)), nc_arg),
                          lambda hs, ws: (nc_arg,))
        return _RaggedPlan(host, host.to(device) if device is not None else None)
    return _cached_plan(_ragged_plans, _RAGGED_PLANS_KEPT, (tuple(shapes), tuple(channels), bool(has_mask), nc_arg, device), build)


class RaggedBytes:
    """B byte images of different sizes in ONE buffer (the arenas of include/curl_hip_ragged.h): image i's H_i x W_i x C_i
    bytes start `offsets[i]` bytes into `arena`, every offset a multiple of 16, the images in index order with only the
    padding that needs.  The same class carries the images (C = 3 | 4), their 'L' masks (C = 1, [H,W]) and the outputs (C = 3).
    `image(i)[None]` is what ops.encoder_view_u8hwc takes."""

    def __init__(self, arena, shapes, offsets, channels):
        self.arena, self.shapes, self.offsets, self.channels = arena, list(shapes), list(offsets), list(channels)

    def __len__(self):
        return len(self.shapes)

    @property
    def device(self):
        return self.arena.device

    @staticmethod
    def layout(shapes, channels):
        """-> (offsets, arena bytes) of the shape list, from the library's plan.  channels: all 1 (masks), or 3 | 4 per image."""
        shapes, channels = [(int(h), int(w)) for h, w in shapes], [int(c) for c in channels]
        if not shapes:
            return [], 0
        for (h, w), c in zip(shapes, channels):
            if h <= 0 or w <= 0:
                raise ValueError(f"an image of a ragged batch has a zero dimension: {(h, w)}")
        masks = all(c == 1 for c in channels)
        if not masks and any(c not in (3, 4) for c in channels):
            raise ValueError(f"the images of a ragged batch are uint8 [H,W,3|4] (masks: all [H,W]), got channels {channels}")
        plan = _ragged_plan(shapes, [3] * len(shapes) if masks else channels, masks, 0, None)
        return (plan.mask_off, plan.mask_bytes) if masks else (plan.img_off, plan.img_bytes)

    @classmethod
    def pack(cls, images, device=None):
        """A list of uint8 [H,W,3|4] images (or of [H,W] masks), numpy arrays or tensors on the host or the device, each
        copied straight into its slice of one arena on `device` (None: the first tensor's device, else the host)."""
        import numpy as np
        ts = []
        for k, x in enumerate(images):
            t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
            if t.dtype != torch.uint8 or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] not in (3, 4)):
                raise ValueError(f"image {k} of a ragged batch must be uint8 [H,W,3|4] (a mask: [H,W]), got {t.dtype} {tuple(t.shape)}")
            if t.numel() == 0:
                raise ValueError(f"image {k} of a ragged batch has a zero dimension: {tuple(t.shape)}")
            ts.append(t)
        if len({t.dim() for t in ts}) > 1:
            raise ValueError("a ragged batch holds images ([H,W,3|4]) or masks ([H,W]), not both")
        if device is None:
            device = ts[0].device if ts else torch.device("cpu")
        shapes, channels = [tuple(t.shape[:2]) for t in ts], [t.shape[2] if t.dim() == 3 else 1 for t in ts]
        offsets, nbytes = cls.layout(shapes, channels)
        rb = cls(torch.empty(nbytes, dtype=torch.uint8, device=device), shapes, offsets, channels)
        for i, t in enumerate(ts):
            rb.image(i).copy_(t)
        return rb

    def image(self, i):
        """A view of image i: [H,W,C] (masks: [H,W])."""
        (h, w), c, o = self.shapes[i], self.channels[i], self.offsets[i]
        flat = self.arena[o:o + h * w * c]
        return flat.view(h, w) if c == 1 else flat.view(h, w, c)

    def images(self):
        return [self.image(i) for i in range(len(self))]


def _ragged_inputs(images, white_masks, device):
    """The two arenas of a ragged call, checked -> (images, masks or None)."""
    if not isinstance(images, RaggedBytes):  # a list: to the device its tensors are on, else to the coefficients' / knots'
        images = list(images)
        device = next((t.device for t in images if isinstance(t, torch.Tensor) and t.is_cuda), device)
    rb = images if isinstance(images, RaggedBytes) else RaggedBytes.pack(images, device)
    if any(c not in (3, 4) for c in rb.channels):
        raise ValueError("images must be uint8 [H,W,3|4]")
    _need_device(rb.arena, "images")
    wm = None
    if white_masks is not None:
        n = len(white_masks)
        if n != len(rb):
            raise ValueError(f"white_masks must hold one mask per image ({len(rb)}), got {n}")
        wm = white_masks if isinstance(white_masks, RaggedBytes) else RaggedBytes.pack(list(white_masks), rb.device)
        if any(c != 1 for c in wm.channels) or wm.shapes != rb.shapes:
            raise ValueError(f"white_masks must be uint8 [H,W] masks of the images' sizes {rb.shapes}, got {wm.shapes}")
    _need_device(rb.arena, "images")
    if wm is not None:
        _need_device(wm.arena, "white_masks")
        _check_same_device([("images", rb.arena), ("white_masks", wm.arena)])
    return rb, wm


def _ragged_arenas(rb, wm, nc_arg):
    """The plan of the call and its out arena; the callers' arenas are held to the plan's layout."""
    plan = _ragged_plan(rb.shapes, rb.channels, wm is not None, nc_arg, rb.device)
    if rb.offsets != plan.img_off or (wm is not None and wm.offsets != plan.mask_off):
        raise ValueError("the arena's offsets are not the plan's (RaggedBytes.pack lays images out as the library does)")
    if not rb.arena.is_contiguous() or (wm is not None and not wm.arena.is_contiguous()):
        raise ValueError("the arenas must be contiguous")
    out = RaggedBytes(torch.empty(plan.out_bytes, dtype=torch.uint8, device=rb.device), rb.shapes, plan.out_off, [3] * len(rb))
    return plan, out


def _ragged_empty(images, device):
    if isinstance(images, RaggedBytes):
        return len(images) == 0, images.device
    return len(images) == 0, device


def _mask_args(wm):
    """The mask arena's two arguments of a ragged entry: (pointer, bytes), (0, 0) without masks."""
    return (0, 0) if wm is None else (wm.arena.data_ptr(), wm.arena.numel())


def _ragged_sizes(x):
    """The shapes of the images or masks of a ragged call, as given: a RaggedBytes' or a list's."""
    return [tuple(s) for s in x.shapes] if isinstance(x, RaggedBytes) else [tuple(t.shape) for t in x]


def _ragged_fg_masks(images, fg_masks):
    """The foreground entries' masks, held to the images before anything is packed or uploaded: required, one uint8 [H,W]
    mask of each image's size (_ragged_inputs holds the packed arenas to the same)."""
    if fg_masks is None:
        raise ValueError("fg_masks is required (one uint8 [H,W] 'L' mask per image)")
    want, got = [s[:2] for s in _ragged_sizes(images)], _ragged_sizes(fg_masks)
    if len(got) != len(want):
        raise ValueError(f"fg_masks must hold one mask per image ({len(want)}), got {len(got)}")
    if got != want:
        raise ValueError(f"fg_masks must be uint8 [H,W] masks of the images' sizes {want}, got {got}")
    if not isinstance(fg_masks, RaggedBytes) and any(not str(t.dtype).endswith("uint8") for t in fg_masks):
        raise ValueError(f"fg_masks must be uint8 [H,W] masks, got {[str(t.dtype) for t in fg_masks]}")


def _trispace_u8hwc_ragged(images, coeffs, masks, fg):
    """The two ragged polynomial ops: the plain entry, or with fg the foreground one (its masks required, and checked first)."""
    empty, device = _ragged_empty(images, coeffs.device if isinstance(coeffs, torch.Tensor) else None)
    if fg:
        _ragged_fg_masks(images, masks)
    if empty:
        return RaggedBytes(torch.empty(0, dtype=torch.uint8, device=device), [], [], [])
    lib = _lib.load()
    rb, wm = _ragged_inputs(images, masks, device)
    _check_coeffs(coeffs, len(rb))
    _check_same_device([("images", rb.arena), ("coeffs", coeffs)])
    c = _coeffs32(coeffs, pairs=coeffs.shape[3] == 126)
    nc = _nc_arg(c.shape[3])
    plan, out = _ragged_arenas(rb, wm, nc)
    entry = "curl_trispace_fwd_ragged_fg_u8hwc" if fg else "curl_trispace_fwd_ragged_u8hwc"
    with torch.cuda.device(rb.device):
        rc = getattr(lib, entry)(rb.arena.data_ptr(), rb.arena.numel(), c.data_ptr(), *_mask_args(wm), out.arena.data_ptr(),
                                 out.arena.numel(), plan.host.data_ptr(), plan.dev.data_ptr(), plan.nbytes, nc, 0, _stream(rb.arena))
    _lib.check(rc, entry)
    return out


def _curl_layer_u8hwc_ragged(images, L, R, H, masks, fg):
    """The two ragged curve-layer ops: the plain entry, or with fg the foreground one (its masks required, and checked first)."""
    empty, device = _ragged_empty(images, L.device if isinstance(L, torch.Tensor) else None)
    if fg:
        _ragged_fg_masks(images, masks)
    if empty:
        return (RaggedBytes(torch.empty(0, dtype=torch.uint8, device=device), [], [], []),
                torch.zeros(0, dtype=torch.float32, device=device))
    lib = _lib.load()
    rb, wm = _ragged_inputs(images, masks, device)
    B = len(rb)
    Lc, Rc, Hc, Kl, Kr, Kh, n_knots = _layer_knots(L, R, H, B)
    _check_same_device([("images", rb.arena), ("L", Lc), ("R", Rc), ("H", Hc)])
    plan, out = _ragged_arenas(rb, wm, 0)
    reg = torch.empty(B, dtype=torch.float32, device=rb.device)
    ws, nbytes = _workspace(B, n_knots, rb.device)
    entry = "curl_layer_fwd_ragged_fg_u8hwc" if fg else "curl_layer_fwd_ragged_u8hwc"
    with torch.cuda.device(rb.device):
        rc = getattr(lib, entry)(rb.arena.data_ptr(), rb.arena.numel(), Lc.data_ptr(), Rc.data_ptr(), Hc.data_ptr(), *_mask_args(wm),
                                 out.arena.data_ptr(), out.arena.numel(), reg.data_ptr(), ws.data_ptr(), nbytes, plan.host.data_ptr(),
                                 plan.dev.data_ptr(), plan.nbytes, Kl, Kr, Kh, 0, _stream(rb.arena))
    _lib.check(rc, entry)
    return out, reg


def trispace_forward_u8hwc_ragged(images, coeffs, white_masks=None):
    """trispace_forward_u8hwc for a batch of images of different sizes in one launch per class of images (dword / byte):
    images a RaggedBytes or a list of uint8 [H,W,3|4] (alpha is not read), coeffs [B,3,3,n], white_masks None or one [H,W]
    uint8 mask per image (a RaggedBytes or a list).  -> RaggedBytes of the [H,W,3] outputs; every image's bytes equal
    trispace_forward_u8hwc of that image alone."""
    return _trispace_u8hwc_ragged(images, coeffs, white_masks, False)


def curl_layer_forward_u8hwc_ragged(images, L, R, H, white_masks=None):
    """curl_layer_forward_u8hwc(img, None, L, R, H, white_mask) for a batch of images of different sizes: one curve collapse
    for the B knot rows and one launch per class of images.  -> (RaggedBytes of the [H,W,3] outputs, reg [B]); bytes and reg
    equal the single-image calls'."""
    return _curl_layer_u8hwc_ragged(images, L, R, H, white_masks, False)


def trispace_foreground_u8hwc_ragged(images, coeffs, fg_masks):
    """trispace_forward_u8hwc_ragged with white_masks = fg_masks for segmentation masks, byte for byte the same result:
    wavefronts whose mask bytes are all 0 store white and never read their pixels, workgroups of such wavefronts stage no
    table (curl_trispace_fwd_ragged_fg_u8hwc).  The same inputs, fg_masks required; the cached plan of a shape list is the
    plain call's.  -> RaggedBytes of the [H,W,3] outputs."""
    return _trispace_u8hwc_ragged(images, coeffs, fg_masks, True)


def curl_layer_foreground_u8hwc_ragged(images, L, R, H, fg_masks):
    """curl_layer_forward_u8hwc_ragged with white_masks = fg_masks for segmentation masks, byte for byte the same result and
    the same reg (curl_layer_fwd_ragged_fg_u8hwc).  -> (RaggedBytes of the [H,W,3] outputs, reg [B])."""
    return _curl_layer_u8hwc_ragged(images, L, R, H, fg_masks, True)


# ------------------------------------------------------------------ the score of a ragged batch (include/curl_hip_ragged_score.h)
def _score_shapes(x, name):
    """The [(H, W)] of one side of a score call, held to uint8 [H,W,3] before anything is packed or uploaded."""
    if isinstance(x, RaggedBytes):
        if any(c != 3 for c in x.channels):
            raise ValueError(f"{name} must hold uint8 [H,W,3] images, got channels {x.channels}")
        return [tuple(s) for s in x.shapes]
    shapes = []
    for k, t in enumerate(x):
        shape = tuple(getattr(t, "shape", ()))
        if not str(getattr(t, "dtype", "")).endswith("uint8") or len(shape) != 3 or shape[2] != 3 or 0 in shape:
            raise ValueError(f"image {k} of {name} must be uint8 [H,W,3], got {getattr(t, 'dtype', type(t).__name__)} {shape}")
        shapes.append((int(shape[0]), int(shape[1])))
    return shapes


def _score_masks(masks, shapes):
    """The optional masks of a score call, held to the images: one uint8 [H,W] mask of each image's size."""
    if masks is None:
        return
    if isinstance(masks, RaggedBytes):
        got = [tuple(s) for s in masks.shapes] if all(c == 1 for c in masks.channels) else None
    else:
        masks = list(masks)
        if any(not str(getattr(t, "dtype", "")).endswith("uint8") for t in masks):
            raise ValueError(f"masks must be uint8 [H,W] masks, got {[str(getattr(t, 'dtype', type(t).__name__)) for t in masks]}")
        got = [tuple(t.shape) for t in masks]
    if got != shapes:
        raise ValueError(f"masks must be one uint8 [H,W] mask per image, of the images' sizes {shapes}, got {got}")


def _score_device(a, b):
    """Where the empty result of a score call goes: the device of the side that is a RaggedBytes, else None."""
    return next((x.device for x in (a, b) if isinstance(x, RaggedBytes)), None)


def _score_plan(shapes, has_mask, device):
    """The plan sse_u8hwc_ragged scores by: the op-0 plan of the shape list as RGB images, whose out arena both sides have."""
    return _ragged_plan(shapes, [3] * len(shapes), has_mask, 0, device)


def _score_inputs(a, b, masks, names, get_plan, rgb_off, check=None):
    """The front end of the ops that score one ragged byte batch against another: both sides (names: what the messages call
    them) held to uint8 [H,W,3] images of one shape list and the masks to it, then check(shapes) -- the op's own conditions --
    all before anything is packed or uploaded; the arenas packed onto one device and held to the offsets (plan.<rgb_off>,
    plan.mask_off) of get_plan(shapes, has_mask, device).  -> (a's arena, b's, the masks' or None, the plan); four None for
    an empty batch."""
    shapes = _score_shapes(a, names[0])
    if _score_shapes(b, names[1]) != shapes:
        raise ValueError(f"{names[0]} and {names[1]} must hold images of the same sizes, got {shapes} and {_score_shapes(b, names[1])}")
    _score_masks(masks, shapes)
    if check is not None:
        check(shapes)
    if not shapes:
        return None, None, None, None
    _lib.load()
    ra, wm = _ragged_inputs(a, masks, None)
    rb = b if isinstance(b, RaggedBytes) else RaggedBytes.pack(list(b), ra.device)
    _need_device(rb.arena, names[1])
    _check_same_device([(names[0], ra.arena), (names[1], rb.arena)])
    plan = get_plan(ra.shapes, wm is not None, ra.device)
    off = getattr(plan, rgb_off)
    if ra.offsets != off or rb.offsets != off or (wm is not None and wm.offsets != plan.mask_off):
        raise ValueError("the arena's offsets are not the plan's (RaggedBytes.pack lays images out as the library does)")
    if not ra.arena.is_contiguous() or not rb.arena.is_contiguous() or (wm is not None and not wm.arena.is_contiguous()):
        raise ValueError("the arenas must be contiguous")
    return ra, rb, wm, plan


def sse_u8hwc_ragged(a, b, masks=None):
    """The exact masked squared error of two batches of byte images of different sizes, every image in one pass
    (curl_sse_ragged_u8hwc): a and b a RaggedBytes or a list of uint8 [H,W,3] images of the same shape list, masks None or one
    uint8 [H,W] mask per image (a RaggedBytes or a list).  -> int64 [B,2] on the device: [i,0] the sum over the pixels whose
    mask byte is not 0 (all pixels without masks) and the 3 channels of (a - b)^2, [i,1] the number of those pixels.  Integer
    arithmetic throughout: the same bits on every call, for an image alone or in any company and order."""
    ra, rb, wm, plan = _score_inputs(a, b, masks, ("a", "b"), _score_plan, "out_off")
    if plan is None:
        return torch.zeros((0, 2), dtype=torch.int64, device=_score_device(a, b))
    lib = _lib.load()
    sums = torch.empty((len(ra), 2), dtype=torch.int64, device=ra.device)
    nbytes = lib.curl_ragged_score_workspace_bytes(plan.host.data_ptr())
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=ra.device)
    with torch.cuda.device(ra.device):
        rc = lib.curl_sse_ragged_u8hwc(ra.arena.data_ptr(), ra.arena.numel(), rb.arena.data_ptr(), rb.arena.numel(), *_mask_args(wm),
                                       sums.data_ptr(), sums.numel() * 8, ws.data_ptr(), nbytes, plan.host.data_ptr(),
                                       plan.dev.data_ptr(), plan.nbytes, 0, _stream(ra.arena))
    _lib.check(rc, "curl_sse_ragged_u8hwc")
    return sums


def psnr_u8hwc_ragged(a, b, masks=None):
    """The masked PSNR of every image of a ragged byte batch against its target, float64 [B] on the device:
    10 * log10(255^2 * 3 N / SSE) from sse_u8hwc_ragged's integers (no synchronisation) -- metric.py:35-64 on the bytes / 255,
    without its float32 sum.  nan for an image whose mask keeps no pixel (0 / 0), inf for equal images (1 / 0), as there."""
    sums = sse_u8hwc_ragged(a, b, masks).to(torch.float64)  # exact: both columns are below 2^53
    return 10.0 * torch.log10(255.0 ** 2 * 3.0 * sums[:, 1] / sums[:, 0])


# ------------------------------------------------------------------ MS-SSIM of a ragged batch (include/curl_hip_ragged_msssim.h)
_msssim_ragged_plans = {}  # (shapes, has_mask, device) -> _MsssimRaggedPlan
MSSSIM_MIN_SIDE = 32       # metric.py:185-192 pools once more after the fifth level
# metric.py:86: the five level weights, float32 there and raised to the images' dtype (here: float64)
_MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


class _MsssimRaggedPlan:
    """One MS-SSIM plan of the library's: the host copy (int32), its upload and what the callers read from it."""

    def __init__(self, host, dev, ws_bytes):
        self.host, self.dev, self.ws_bytes = host, dev, ws_bytes
        w = host.numpy()
        hw, dw = _lib.MSSSIM_RAGGED_HEADER_WORDS, _lib.MSSSIM_RAGGED_DESC_WORDS
        B = int(w[1])
        self.nbytes = host.numel() * 4
        self.rgb_bytes, self.mask_bytes = (int(v) for v in w[12:16].view("int64"))
        off = w[hw:hw + B * dw].reshape(B, dw)[:, 4:8].copy().view("int64")  # rgb_off, mask_off per descriptor (index order)
        self.rgb_off, self.mask_off = ([int(v) for v in off[:, k]] for k in range(2))


def _msssim_ragged_plan(shapes, has_mask, device):
    """The MS-SSIM plan of a shape list, built on the host by the library, uploaded once and kept, as the op-0 plan is."""
    return _pyramid_ragged_plan(_msssim_ragged_plans, "msssim", shapes, has_mask, device)


def _pyramid_ragged_plan(cache, kind, shapes, has_mask, device):
    """The plan of curl_<kind>_ragged_plan (kind: msssim | loss; one layout) of a shape list, kept in `cache`."""
    def build():
        host = _host_plan(f"curl_{kind}_ragged_plan", shapes, None, _lib.RAGGED_MAX_IMAGES, (int(bool(has_mask)),))
        ws_bytes = getattr(_lib.load(), f"curl_{kind}_ragged_workspace_bytes")(host.data_ptr())
        return _MsssimRaggedPlan(host, host.to(device), ws_bytes)
    return _cached_plan(cache, _RAGGED_PLANS_KEPT, (tuple(shapes), bool(has_mask), device), build)


def _pyramid_stats_u8hwc_ragged(a, b, masks, window_size, rows, kind, get_plan, names, needs):
    """The body of the two pyramid-statistics ops: curl_<kind>_ragged_u8hwc (kind: msssim | loss) on the plan get_plan gives
    -> float64 [B,rows,5].  names: what the messages call the two sides; needs: what, in them, needs every side >= 32."""
    def check(shapes):
        if window_size not in (1, 3, 5, 7, 9, 11):
            raise ValueError(f"window_size must be odd and 1..11, got {window_size}")
        for k, (h, w) in enumerate(shapes):
            if h < MSSSIM_MIN_SIDE or w < MSSSIM_MIN_SIDE:
                raise ValueError(f"image {k} is {h}x{w}: {needs} needs H, W >= {MSSSIM_MIN_SIDE} (five pyramid levels, each followed by a 2x2 pooling)")
    ra, rb, wm, plan = _score_inputs(a, b, masks, names, get_plan, "rgb_off", check)
    if plan is None:
        return torch.zeros((0, rows, 5), dtype=torch.float64, device=_score_device(a, b))
    entry = f"curl_{kind}_ragged_u8hwc"
    call = getattr(_lib.load(), entry)
    stats = torch.empty((len(ra), rows, 5), dtype=torch.float64, device=ra.device)
    ws = torch.empty(plan.ws_bytes // 8, dtype=torch.float64, device=ra.device)
    with torch.cuda.device(ra.device):
        rc = call(ra.arena.data_ptr(), ra.arena.numel(), rb.arena.data_ptr(), rb.arena.numel(), *_mask_args(wm), stats.data_ptr(),
                  stats.numel() * 8, ws.data_ptr(), plan.ws_bytes, plan.host.data_ptr(), plan.dev.data_ptr(), plan.nbytes, window_size, 0,
                  _stream(ra.arena))
    _lib.check(rc, entry)
    return stats


def msssim_stats_u8hwc_ragged(a, b, masks=None, window_size=11):
    """The MS-SSIM statistics of two batches of byte images of different sizes, the whole batch in six launches
    (curl_msssim_ragged_u8hwc): a and b a RaggedBytes or a list of uint8 [H,W,3] images of the same shape list (every side
    >= 32), masks None or one uint8 [H,W] mask per image.  -> float64 [B,2,5] on the device: [i,0,l] the mean of level l's SSIM
    map of image i, [i,1,l] that of its contrast-structure map -- msssim_stats of bytes / 255 times (mask != 0), without the
    float images.  The same bits on every call, for an image alone or in any company and order."""
    return _pyramid_stats_u8hwc_ragged(a, b, masks, window_size, 2, "msssim", _msssim_ragged_plan, ("a", "b"), "MS-SSIM")


def msssim_from_stats(stats):
    """metric.py:200-207 on [B,2,5] statistics, in their dtype on their device: (x + 1) / 2, the powers by the five weights,
    prod(mcs[:-1]^w[:-1] * ssims[-1]^w[-1]) -- the reference's quirk kept: the last factor enters four times."""
    w = torch.tensor(_MSSSIM_WEIGHTS, dtype=torch.float32).to(device=stats.device, dtype=stats.dtype)
    x = (stats + 1) / 2
    pow1, pow2 = x[:, 1] ** w, x[:, 0] ** w
    return torch.prod(pow1[:, :-1] * pow2[:, -1].reshape(-1, 1), dim=1)


def msssim_u8hwc_ragged(a, b, masks=None, window_size=11):
    """The MS-SSIM of every image of a ragged byte batch against its target, float64 [B] on the device: metric.py:200-207 on
    msssim_stats_u8hwc_ragged's statistics, in float64, without a synchronisation."""
    return msssim_from_stats(msssim_stats_u8hwc_ragged(a, b, masks, window_size))


# ------------------------------------------------------------------ CURLLoss of a ragged batch (include/curl_hip_ragged_loss.h)
_loss_ragged_plans = {}  # (shapes, has_mask, device) -> _MsssimRaggedPlan (the layout is the MS-SSIM plan's)


def _loss_ragged_plan(shapes, has_mask, device):
    """The loss plan of a shape list, built on the host by the library, uploaded once and kept, as the MS-SSIM plan is."""
    return _pyramid_ragged_plan(_loss_ragged_plans, "loss", shapes, has_mask, device)


def loss_stats_u8hwc_ragged(pred, target, masks=None, window_size=11):
    """The statistics of the reference's CURLLoss (model.py:78-116) of two batches of byte images of different sizes, the whole
    batch in six launches (curl_loss_ragged_u8hwc): pred and target a RaggedBytes or a list of uint8 [H,W,3] images of the same
    shape list (every side >= 32), masks None or one uint8 [H,W] mask per image.  -> float64 [B,3,5] on the device: [i,0] the
    raw sums over the pixels whose mask byte is not 0 of |p - t|, the cosine similarity, |Lab_p - Lab_t| and |cone_p - cone_t|,
    then their number N; [i,1,l] / [i,2,l] the means of level l's SSIM and contrast-structure maps of the clamped-L planes.
    The prediction is the BYTES / 255 -- an output file's pixels, not a network's unrounded float output.  The same bits on every
    call, for an image alone or in any company and order."""
    return _pyramid_stats_u8hwc_ragged(pred, target, masks, window_size, 3, "loss", _loss_ragged_plan, ("pred", "target"),
                                       "the loss's MS-SSIM term")


def curl_loss_from_stats(stats, shapes):
    """model.py:89-116 on [B,3,5] statistics and the images' [(H, W)], in float64 on the statistics' device (a CPU tensor too; no
    synchronisation) -> float64 [B], every image's loss as CURLLoss()(pred[None], target[None], mask[None]) gives it: rgb, lab,
    hsv = S / (3 N); cosine = 1 - (S_cos + (H W - N)) / (H W) -- a masked-out pixel has a cosine similarity of 0 and the mean runs
    over all pixels --; ssim = 1 - msssim_from_stats(rows 1, 2); loss = (rgb + cosine + lab + hsv + 10 ssim) / 5.  N = 0 gives
    nan, as the reference's 0 / 0 does."""
    stats = stats.to(torch.float64)
    if stats.dim() != 3 or tuple(stats.shape[1:]) != (3, 5) or stats.shape[0] != len(shapes):
        raise ValueError(f"stats must be [B,3,5] with one (H, W) per image, got {tuple(stats.shape)} and {len(shapes)} shapes")
    hw = torch.tensor([float(h * w) for h, w in shapes], dtype=torch.float64).to(stats.device)
    S, n = stats[:, 0, :4], stats[:, 0, 4]
    rgb, lab, hsv = (S[:, k] / (3.0 * n) for k in (0, 2, 3))
    cosine = 1.0 - (S[:, 1] + (hw - n)) / hw
    ssim = 1.0 - msssim_from_stats(stats[:, 1:])
    return (rgb + cosine + lab + hsv + 10.0 * ssim) / 5.0


def curl_loss_u8hwc_ragged(pred, target, masks=None):
    """The reference's CURLLoss of every image of a ragged byte batch against its target, float64 [B] on the device:
    curl_loss_from_stats on loss_stats_u8hwc_ragged's statistics.  It is the criterion of the bytes written (byte / 255)."""
    stats = loss_stats_u8hwc_ragged(pred, target, masks)
    return curl_loss_from_stats(stats, _score_shapes(pred, "pred"))


_view_plans = {}  # (H, W, size, device) -> the uploaded plan (int32, a few dozen KB each)
_VIEW_PLANS_KEPT = 16


def _view_plan(H, W, size, device):
    """The coefficient tables of one shape on the device: built on the host by the library, uploaded once, kept for the
    next frames of that shape (the oldest of more than sixteen shapes is dropped)."""
    key = (H, W, size, device)
    plan = _view_plans.get(key)
    if plan is None:
        lib = _lib.load()
        nbytes = lib.curl_encoder_view_plan_bytes(H, W, size)
        host = torch.empty(max(nbytes, 4) // 4, dtype=torch.int32)
        _lib.check(lib.curl_encoder_view_plan(H, W, size, host.data_ptr(), nbytes), "curl_encoder_view_plan")
        if len(_view_plans) >= _VIEW_PLANS_KEPT:
            del _view_plans[next(iter(_view_plans))]
        plan = _view_plans[key] = host.to(device)
    return plan


@_one_device
def encoder_view_u8hwc(img_u8, mask_u8=None, size=_lib.VIEW_SIZE_DEFAULT):
    """The encoder's input as the reference makes it (infer.py:32-41), from the decoded bytes in one launch: torchvision's
    Resize([size]) + CenterCrop((size, size)) -- Pillow's 8-bit antialiased bilinear resample, bit for bit -- then to_tensor.
    img_u8 uint8 [B,H,W,3|4] (alpha is not read), mask_u8 uint8 [B,H,W] or None
    -> (view float32 [B,3,size,size], mask_view float32 [B,1,size,size] = (resampled mask byte > 0), or None)."""
    lib = _lib.load()
    _need_device(img_u8, "img_u8")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[3] not in (3, 4):
        raise ValueError(f"img_u8 must be uint8 [B,H,W,3|4], got {img_u8.dtype} {tuple(img_u8.shape)}")
    if img_u8.numel() == 0:
        raise ValueError(f"img_u8 is empty: {tuple(img_u8.shape)}")
    x = img_u8.contiguous()
    B, H, W, C = x.shape
    m = None
    if mask_u8 is not None:
        _need_device(mask_u8, "mask_u8")
        if mask_u8.dtype != torch.uint8 or tuple(mask_u8.shape) != (B, H, W):
            raise ValueError(f"mask_u8 must be uint8 [B,H,W] ('L' image), got {mask_u8.dtype} {tuple(mask_u8.shape)}")
        m = mask_u8.contiguous()
    size = int(size)
    plan = _view_plan(H, W, size, x.device)
    view = torch.empty(B, 3, size, size, dtype=torch.float32, device=x.device)
    mview = torch.empty(B, 1, size, size, dtype=torch.float32, device=x.device) if m is not None else None
    rc = lib.curl_encoder_view_u8hwc(x.data_ptr(), C, _ptr(m), plan.data_ptr(), plan.numel() * 4, view.data_ptr(), _ptr(mview),
                                     B, H, W, size, 0, _stream(x))
    _lib.check(rc, "curl_encoder_view_u8hwc")
    return view, mview


# ------------------------------------------------------------------ the views of a ragged batch (include/curl_hip_view_ragged.h)
_view_ragged_plans = {}  # (shapes, channels, has_mask, size, device) -> _ViewRaggedPlan
_VIEW_RAGGED_PLANS_KEPT = 16


class _ViewRaggedPlan:
    """One plan of the library's: the host copy (int32), its upload and what the caller reads from it -- the arena sizes and
    the per-image offsets, from the descriptors as the header documents them."""

    def __init__(self, host, dev):
        self.host, self.dev = host, dev
        w = host.numpy()
        hw, dw = _lib.VIEW_RAGGED_HEADER_WORDS, _lib.VIEW_RAGGED_DESC_WORDS
        B = int(w[1])
        self.nbytes = host.numel() * 4
        self.img_bytes, self.mask_bytes = (int(v) for v in w[8:12].view("int64"))
        off = w[hw:hw + B * dw].reshape(B, dw)[:, 20:24].copy().view("int64")  # img_off, mask_off per descriptor (index order)
        self.img_off, self.mask_off = ([int(v) for v in off[:, k]] for k in range(2))


def _view_ragged_plan(shapes, channels, has_mask, size, device):
    """The plan of a shape list at one size, built on the host by the library, uploaded once and kept; the oldest of more than
    sixteen is dropped."""
    def build():
        host = _host_plan("curl_encoder_view_ragged_plan", shapes, channels, _lib.VIEW_RAGGED_MAX_IMAGES, (int(bool(has_mask)), size),
                          lambda hs, ws: (hs, ws, size))
        return _ViewRaggedPlan(host, host.to(device))
    return _cached_plan(_view_ragged_plans, _VIEW_RAGGED_PLANS_KEPT, (tuple(shapes), tuple(channels), bool(has_mask), size, device), build)


def encoder_view_u8hwc_ragged(images, masks=None, size=_lib.VIEW_SIZE_DEFAULT):
    """encoder_view_u8hwc for a batch of images of different sizes in ONE launch: images a RaggedBytes or a list of uint8
    [H,W,3|4] (alpha is not read), masks None or one [H,W] uint8 mask per image (a RaggedBytes or a list).
    -> (view float32 [B,3,size,size], mask_view float32 [B,1,size,size] or None); image i's view equals encoder_view_u8hwc of
    that image alone, bit for bit.  The arenas are the ones the *_u8hwc_ragged ops take."""
    size = int(size)
    empty, device = _ragged_empty(images, None)
    if empty:
        return (torch.empty(0, 3, size, size, dtype=torch.float32, device=device),
                None if masks is None else torch.empty(0, 1, size, size, dtype=torch.float32, device=device))
    lib = _lib.load()
    if masks is not None:  # (before anything is packed or uploaded; _ragged_inputs holds the packed arenas to the same)
        want, got = [s[:2] for s in _ragged_sizes(images)], _ragged_sizes(masks)
        if len(got) != len(want):
            raise ValueError(f"masks must hold one mask per image ({len(want)}), got {len(got)}")
        if got != want:
            raise ValueError(f"masks must be uint8 [H,W] masks of the images' sizes {want}, got {got}")
    rb, wm = _ragged_inputs(images, masks, device)
    plan = _view_ragged_plan(rb.shapes, rb.channels, wm is not None, size, rb.device)
    if rb.offsets != plan.img_off or (wm is not None and wm.offsets != plan.mask_off):
        raise ValueError("the arena's offsets are not the plan's (RaggedBytes.pack lays images out as the library does)")
    if not rb.arena.is_contiguous() or (wm is not None and not wm.arena.is_contiguous()):
        raise ValueError("the arenas must be contiguous")
    B = len(rb)
    view = torch.empty(B, 3, size, size, dtype=torch.float32, device=rb.device)
    mview = torch.empty(B, 1, size, size, dtype=torch.float32, device=rb.device) if wm is not None else None
    with torch.cuda.device(rb.device):
        rc = lib.curl_encoder_view_ragged_u8hwc(rb.arena.data_ptr(), rb.arena.numel(), *_mask_args(wm), plan.host.data_ptr(),
                                                plan.dev.data_ptr(), plan.nbytes, view.data_ptr(), _ptr(mview), size, 0, _stream(rb.arena))
    _lib.check(rc, "curl_encoder_view_ragged_u8hwc")
    return view, mview


def _planes(t, name):
    _need_device(t, name)
    if t.dim() != 4 or t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32 [B,C,H,W], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


@_one_device
def msssim_stats(a, b, window_size=11):
    """MSSSIMMetric.compute_ssim over the five pyramid levels (metric.py:120-166,185-192) in five launches.
    a, b [B,C,H,W] -> (ssims [B,5], mcs [B,5]): per level, the per-image means of the SSIM and contrast-structure maps."""
    lib = _lib.load()
    a, b = _planes(a, "img1"), _planes(b, "img2")
    if a.shape != b.shape:
        raise RuntimeError(f"Input images must have the same shape ({tuple(a.shape)} vs. {tuple(b.shape)}).")
    B, C, H, W = a.shape
    nbytes = lib.curl_msssim_scratch_bytes(B, C, H, W)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=a.device)
    ssims = torch.empty(B, 5, dtype=torch.float32, device=a.device)
    mcs = torch.empty_like(ssims)
    rc = lib.curl_msssim_fwd_f32(a.data_ptr(), b.data_ptr(), ssims.data_ptr(), mcs.data_ptr(), scratch.data_ptr(), nbytes,
                                 B, C, H, W, window_size, _stream(a))
    _lib.check(rc, "curl_msssim_fwd_f32")
    return ssims, mcs


@_one_device
def msssim_stats_backward(a, b, g_ssims, g_mcs, window_size=11):
    """d loss / d a of msssim_stats, given d loss / d ssims and d loss / d mcs ([B,5] each)."""
    lib = _lib.load()
    a, b = _planes(a, "img1"), _planes(b, "img2")
    B, C, H, W = a.shape
    gs = g_ssims.to(torch.float32).contiguous()
    gc = g_mcs.to(torch.float32).contiguous()
    nbytes = lib.curl_msssim_scratch_bytes(B, C, H, W)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=a.device)
    grad = torch.empty_like(a)
    rc = lib.curl_msssim_bwd_f32(a.data_ptr(), b.data_ptr(), gs.data_ptr(), gc.data_ptr(), grad.data_ptr(),
                                 scratch.data_ptr(), nbytes, B, C, H, W, window_size, _stream(a))
    _lib.check(rc, "curl_msssim_bwd_f32")
    return grad


@_one_device
def psnr_per_image(a, b, mask=None, max_intensity=1.0):
    """metric.py:35-62 per image: masked PSNR [B] (NaN where an image has no unmasked pixel or zero error -> inf)."""
    lib = _lib.load()
    a, b = _image(a, "a"), _image(b, "b")
    if a.shape != b.shape:
        raise ValueError("a and b must have the same shape")
    m, kind = _mask(mask, a)
    B, _, H, W = a.shape
    out = torch.empty(B, dtype=torch.float32, device=a.device)
    nbytes = lib.curl_psnr_scratch_bytes(B, H, W)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=a.device)
    rc = lib.curl_psnr_f32(a.data_ptr(), b.data_ptr(), _ptr(m), kind, out.data_ptr(), scratch.data_ptr(), nbytes,
                           B, H, W, float(max_intensity), _stream(a))
    _lib.check(rc, "curl_psnr_f32")
    return out


@_one_device
def loss_term_sums(pred, target, mask, want_L=True):
    """Per-image sums of the CURLLoss pointwise terms (model.py:89-109): [B,5] float64 =
    (sum|p-t|, sum cos_sim, sum|lab|, sum|hsv cone|, sum mask), plus the clamped L planes for MS-SSIM."""
    lib = _lib.load()
    pred, target = _image(pred, "pred"), _image(target, "target")
    if pred.shape != target.shape:
        raise ValueError("pred and target must have the same shape")
    m, kind = _mask(mask, pred)
    B, _, H, W = pred.shape
    sums = torch.empty(B, 5, dtype=torch.float64, device=pred.device)
    Lp = torch.empty(B, 1, H, W, dtype=torch.float32, device=pred.device) if want_L else None
    Lt = torch.empty_like(Lp) if want_L else None
    nbytes = lib.curl_loss_terms_scratch_bytes(B, H, W)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=pred.device)
    rc = lib.curl_loss_terms_f32(pred.data_ptr(), target.data_ptr(), _ptr(m), kind, sums.data_ptr(), _ptr(Lp), _ptr(Lt),
                                 scratch.data_ptr(), nbytes, B, H, W, _stream(pred))
    _lib.check(rc, "curl_loss_terms_f32")
    return sums, Lp, Lt


@_one_device
def layer_loss_forward(img, mask, L, R, H, target, want_L=True):
    """The train step's forward in one pass (main.py:283-285): CURLLayer.forward (model.py:137-176) and CURLLoss' pointwise
    terms (model.py:89-109) on the prediction while it is in registers -- curl_layer_loss_fwd_f32.
    -> (out, reg[B], sums [B,5] float64, L_pred, L_target, workspace): what curl_layer_forward(..., return_workspace=True) and
    loss_term_sums(out, target, mask) return, the same bits, with one mask for both."""
    lib = _lib.load()
    img, target = _image(img), _image(target, "target")
    if img.shape != target.shape:
        raise ValueError("img and target must have the same shape")
    B, _, Hh, W = img.shape
    Lc, Rc, Hc, Kl, Kr, Kh, n_knots = _layer_knots(L, R, H, B)
    m, kind = _mask(mask, img)
    out = torch.empty_like(img)
    reg = torch.empty(B, dtype=torch.float32, device=img.device)
    sums = torch.empty(B, 5, dtype=torch.float64, device=img.device)
    Lp = torch.empty(B, 1, Hh, W, dtype=torch.float32, device=img.device) if want_L else None
    Lt = torch.empty_like(Lp) if want_L else None
    ws, nbytes = _workspace(B, n_knots, img.device)
    sbytes = lib.curl_loss_terms_scratch_bytes(B, Hh, W)
    scratch = torch.empty(sbytes // 4, dtype=torch.float32, device=img.device)
    rc = lib.curl_layer_loss_fwd_f32(img.data_ptr(), _ptr(m), kind, Lc.data_ptr(), Rc.data_ptr(), Hc.data_ptr(), target.data_ptr(),
                                     out.data_ptr(), reg.data_ptr(), sums.data_ptr(), _ptr(Lp), _ptr(Lt), ws.data_ptr(), nbytes,
                                     scratch.data_ptr(), sbytes, B, Hh, W, Kl, Kr, Kh, 0, _stream(img))
    _lib.check(rc, "curl_layer_loss_fwd_f32")
    return out, reg, sums, Lp, Lt, ws


@_one_device
def loss_terms_backward(pred, target, mask, weights, grad_L_pred=None):
    """d(sum_k weights[k] * sum_k-th pointwise sum + <grad_L_pred, L_pred>) / d pred.  weights: device float32 [4]."""
    lib = _lib.load()
    pred, target = _image(pred, "pred"), _image(target, "target")
    m, kind = _mask(mask, pred)
    B, _, H, W = pred.shape
    w = weights.to(torch.float32).contiguous()
    g = None if grad_L_pred is None else grad_L_pred.to(torch.float32).contiguous()
    out = torch.empty_like(pred)
    rc = lib.curl_loss_terms_bwd_f32(pred.data_ptr(), target.data_ptr(), _ptr(m), kind, w.data_ptr(), _ptr(g),
                                     out.data_ptr(), B, H, W, _stream(pred))
    _lib.check(rc, "curl_loss_terms_bwd_f32")
    return out
