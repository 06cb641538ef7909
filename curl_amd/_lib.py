"""ctypes binding of libcurlhip.so (include/curl_hip.h).

There is deliberately NO fallback: if the HIP library is missing the import of any
op fails loudly.  The CPU arithmetic of this path lives in the reference (and in
oracle/, which is test infrastructure); nothing here routes through either.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CURL_HIP_LIB", os.path.join(_HERE, "lib", "libcurlhip.so"))

# include/curl_hip.h
MASK_NONE, MASK_U8, MASK_F32 = 0, 1, 2
F_EXACT_ORDER = 0x1
F_PWL = 0x2
F_RESIDUAL_ONLY = 0x4
F_TUNE_UNROLL_SHIFT = 8
F_TUNE_BLOCK_SHIFT = 11
F_TUNE_XCD_SHIFT = 13
F_TUNE_OCC_SHIFT = 19  # resident workgroups per CU: 0 = per-operator default, 1 = no cap, 2..7
F_TUNE_PREP_SHIFT = 23  # where the curves are collapsed: 0 = by launch size, 1 = a launch of its own, 2 = inside the kernel
F_TUNE_NO_NT = 0x8000
F_DIAG_NO_MEM = 0x10000
F_DIAG_SKIP_PREP = 0x20000
F_WS_READY = 0x40000
F_MASK_FIRST = 0x400000  # foreground masks: fully masked-out wavefronts never read their pixels
MAX_KNOTS = 256


def poly_vars(num_variables, degree):
    """include/curl_hip_poly.h CURL_POLY_VARS(V, degree): curl_poly_layer_f32's num_variables with the polynomial degree in the
    high 16 bits (a plain V is degree 4; degree 0 packs a value the library refuses)."""
    return num_variables | ((degree if degree > 0 else 0x7fff) << 16)


def poly_coeffs(num_coeffs, order):
    """include/curl_hip_poly.h CURL_POLY_COEFFS(num_coeffs, order): the curl_trispace_fwd_* entries' num_coeffs with the
    polynomial order in the high 16 bits (a plain 126 | 35 is order 4)."""
    return num_coeffs | ((order if order > 0 else 0x7fff) << 16)

_c_f = ctypes.c_void_p  # device pointers travel as integers
_i = ctypes.c_int
_u = ctypes.c_uint
_sz = ctypes.c_size_t

# name -> (restype, argtypes); this table is also what tests/test_abi.py checks against the header
SIGNATURES = {
    "curl_version": (_i, []),
    "curl_last_error": (ctypes.c_char_p, []),
    "curl_workspace_bytes": (_sz, [_i, _i]),
    "curl_apply_curve_f32": (_i, [_c_f, _c_f, _c_f, _c_f, _i, _i, _i, _i, _i, _i, _u, _c_f]),
    "curl_adjust_rgb_f32": (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _sz, _i, _i, _i, _i, _u, _c_f]),
    "curl_adjust_lab_f32": (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _sz, _i, _i, _i, _i, _u, _c_f]),
    "curl_adjust_hsv_f32": (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _sz, _i, _i, _i, _i, _u, _c_f]),
    "curl_rgb2lab_f32": (_i, [_c_f, _c_f, _i, _i, _i, _u, _c_f]),
    "curl_lab2rgb_f32": (_i, [_c_f, _c_f, _i, _i, _i, _u, _c_f]),
    "curl_rgb2hsv_f32": (_i, [_c_f, _c_f, _i, _i, _i, _u, _c_f]),
    "curl_hsv2rgb_f32": (_i, [_c_f, _c_f, _i, _i, _i, _u, _c_f]),
    "curl_lab_stage_f32": (_i, [_c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _sz, _i, _i, _i, _i, _u, _c_f]),
    "curl_hsv_stage_f32": (_i, [_c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _sz, _i, _i, _i, _i, _u, _c_f]),
    "curl_layer_fwd_f32": (_i, [_c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _sz,
                                _i, _i, _i, _i, _i, _i, _u, _c_f]),
    "curl_layer_fwd_slab_f32": (_i, [_c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _sz,
                                     _i, _i, _i, _i, _i, _i, _i, _i, _u, _c_f]),
    "curl_layer_bwd_scratch_bytes": (_sz, [_i, _i, _i]),
    "curl_layer_bwd_f32": (_i, [_c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f,
                                _c_f, _sz, _c_f, _sz, _i, _i, _i, _i, _i, _i, _u, _c_f]),
    "curl_layer_pwl_bwd_scratch_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "curl_layer_pwl_bwd_f32": (_i, [_c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f,
                                    _c_f, _sz, _c_f, _sz, _i, _i, _i, _i, _i, _i, _u, _c_f]),
    # backward of the stand-alone curve ops, converters and fused stages
    "curl_adjust_rgb_bwd_f32": (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _sz, _c_f, _sz, _i, _i, _i, _i, _u, _c_f]),
    "curl_adjust_lab_bwd_f32": (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _sz, _c_f, _sz, _i, _i, _i, _i, _u, _c_f]),
    "curl_adjust_hsv_bwd_f32": (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _sz, _c_f, _sz, _i, _i, _i, _i, _u, _c_f]),
    "curl_rgb2lab_bwd_f32": (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _u, _c_f]),
    "curl_lab2rgb_bwd_f32": (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _u, _c_f]),
    "curl_rgb2hsv_bwd_f32": (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _u, _c_f]),
    "curl_hsv2rgb_bwd_f32": (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _u, _c_f]),
    "curl_lab_stage_bwd_f32": (_i, [_c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _sz, _c_f, _sz, _i, _i, _i, _i, _u,
                                    _c_f]),
    "curl_hsv_stage_bwd_f32": (_i, [_c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _sz, _c_f, _sz, _i, _i, _i, _i, _u,
                                    _c_f]),
    "curl_trispace_fwd_f32": (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _u, _c_f]),
    "curl_trispace_fwd_slab_f32": (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _i, _i, _u, _c_f]),
    "curl_trispace_fwd_u8hwc": (_i, [_c_f, _c_f, _c_f, _c_f, _i, _i, _i, _i, _u, _c_f]),
    "curl_layer_fwd_u8hwc": (_i, [_c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _sz, _i, _i, _i, _i, _i, _i,
                                  _u, _c_f]),
    "curl_trispace_bwd_scratch_bytes": (_sz, [_i, _i, _i, _i]),
    "curl_trispace_bwd_f32": (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _sz, _i, _i, _i, _i, _u, _c_f]),
    "curl_poly_layer_f32": (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _c_f]),
    "curl_poly_layer_bwd_scratch_bytes": (_sz, [_i, _i, _i, _i]),
    "curl_poly_layer_bwd_f32": (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _sz, _i, _i, _i, _i, _u, _c_f]),
    "curl_u8hwc_to_f32chw": (_i, [_c_f, _c_f, _i, _i, _i, _i, _c_f]),
    "curl_f32chw_to_u8hwc": (_i, [_c_f, _c_f, _i, _i, _i, _c_f]),
    "curl_psnr_scratch_bytes": (_sz, [_i, _i, _i]),
    "curl_psnr_f32": (_i, [_c_f, _c_f, _c_f, _i, _c_f, _c_f, _sz, _i, _i, _i, ctypes.c_float, _c_f]),
    "curl_msssim_scratch_bytes": (_sz, [_i, _i, _i, _i]),
    "curl_msssim_fwd_f32": (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _sz, _i, _i, _i, _i, _i, _c_f]),
    "curl_msssim_bwd_f32": (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _sz, _i, _i, _i, _i, _i, _c_f]),
    "curl_loss_terms_scratch_bytes": (_sz, [_i, _i, _i]),
    "curl_loss_terms_f32": (_i, [_c_f, _c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _sz, _i, _i, _i, _c_f]),
    "curl_loss_terms_bwd_f32": (_i, [_c_f, _c_f, _c_f, _i, _c_f, _c_f, _c_f, _i, _i, _i, _c_f]),
    "curl_layer_loss_fwd_f32": (_i, [_c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _sz, _c_f, _sz,
                                     _i, _i, _i, _i, _i, _i, _u, _c_f]),
    "curl_compose_white_u8hwc": (_i, [_c_f, _c_f, _i, _c_f, _i, _i, _i, _c_f]),
}

# include/curl_hip_grad.h: the entry points declared beside curl_hip.h (bound by load() with the table above; a table of its
# own because tests/test_abi.py holds SIGNATURES to curl_hip.h's declarations)
SIGNATURES_GRAD = {
    "curl_trispace_bwd_img_f32": (_i, [_c_f, _c_f, _c_f, _c_f, _i, _i, _i, _i, _u, _c_f]),
}

# include/curl_hip_view.h: the encoder's view from image bytes (a third table, for the same reason; the two plan functions take
# and fill HOST memory and make no HIP call)
SIGNATURES_VIEW = {
    "curl_encoder_view_plan_bytes": (_sz, [_i, _i, _i]),
    "curl_encoder_view_plan": (_i, [_i, _i, _i, _c_f, _sz]),
    "curl_encoder_view_u8hwc": (_i, [_c_f, _i, _c_f, _c_f, _sz, _c_f, _c_f, _i, _i, _i, _i, _u, _c_f]),
}
VIEW_SIZE_DEFAULT = 320  # CURL_VIEW_SIZE_DEFAULT

# include/curl_hip_fg.h: the foreground-aware byte paths (a fourth table, for the same reason)
SIGNATURES_FG = {
    "curl_trispace_fwd_fg_u8hwc": (_i, [_c_f, _i, _c_f, _c_f, _c_f, _i, _i, _i, _i, _u, _c_f]),
    "curl_layer_fwd_fg_u8hwc": (_i, [_c_f, _i, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _sz, _i, _i, _i, _i, _i, _i, _u, _c_f]),
}

# include/curl_hip_ragged.h: a batch of images of different sizes in one launch per class (a fifth table, for the same reason;
# the plan functions take and fill HOST memory and make no HIP call)
SIGNATURES_RAGGED = {
    "curl_ragged_plan_bytes": (_sz, [_i, _i]),
    "curl_ragged_plan": (_i, [_i, _c_f, _c_f, _c_f, _i, _i, _c_f, _sz]),
    "curl_ragged_arena_bytes": (_i, [_c_f, _c_f, _c_f, _c_f]),
    "curl_trispace_fwd_ragged_u8hwc": (_i, [_c_f, _sz, _c_f, _c_f, _sz, _c_f, _sz, _c_f, _c_f, _sz, _i, _u, _c_f]),
    "curl_layer_fwd_ragged_u8hwc": (_i, [_c_f, _sz, _c_f, _c_f, _c_f, _c_f, _sz, _c_f, _sz, _c_f, _c_f, _sz, _c_f, _c_f, _sz,
                                         _i, _i, _i, _u, _c_f]),
}
# the plan's layout (int32 words): CURL_RAGGED_ALIGN, _STAMP, _HEADER_WORDS, _DESC_WORDS, _MAX_IMAGES
RAGGED_ALIGN, RAGGED_STAMP, RAGGED_HEADER_WORDS, RAGGED_DESC_WORDS, RAGGED_MAX_IMAGES = 16, 0x52474731, 32, 16, 65535

# include/curl_hip_view_ragged.h: the encoder's views of a batch of images of different sizes in one launch (a sixth table,
# for the same reason -- tests/test_encoder_view_abi.py holds SIGNATURES_VIEW to the three entries of curl_hip_view.h; the plan
# functions take and fill HOST memory and make no HIP call)
SIGNATURES_VIEW_RAGGED = {
    "curl_encoder_view_ragged_plan_bytes": (_sz, [_i, _c_f, _c_f, _i]),
    "curl_encoder_view_ragged_plan": (_i, [_i, _c_f, _c_f, _c_f, _i, _i, _c_f, _sz]),
    "curl_encoder_view_ragged_u8hwc": (_i, [_c_f, _sz, _c_f, _sz, _c_f, _c_f, _sz, _c_f, _c_f, _i, _u, _c_f]),
}
# the plan's layout (int32 words): CURL_VIEW_RAGGED_STAMP, _HEADER_WORDS, _DESC_WORDS, _MAX_IMAGES
VIEW_RAGGED_STAMP, VIEW_RAGGED_HEADER_WORDS, VIEW_RAGGED_DESC_WORDS, VIEW_RAGGED_MAX_IMAGES = 0x52565031, 32, 32, 65535

# include/curl_hip_ragged_fg.h: the ragged byte paths, foreground-aware (a seventh table, for the same reason --
# tests/test_ragged_abi.py holds SIGNATURES_RAGGED to the five entries of curl_hip_ragged.h; the argument lists are the siblings')
SIGNATURES_RAGGED_FG = {
    "curl_trispace_fwd_ragged_fg_u8hwc": (_i, list(SIGNATURES_RAGGED["curl_trispace_fwd_ragged_u8hwc"][1])),
    "curl_layer_fwd_ragged_fg_u8hwc": (_i, list(SIGNATURES_RAGGED["curl_layer_fwd_ragged_u8hwc"][1])),
}

# include/curl_hip_ragged_score.h: the exact score of a ragged byte batch (an eighth table, for the same reason; the workspace
# query takes HOST memory and makes no HIP call)
SIGNATURES_RAGGED_SCORE = {
    "curl_ragged_score_workspace_bytes": (_sz, [_c_f]),
    "curl_sse_ragged_u8hwc": (_i, [_c_f, _sz, _c_f, _sz, _c_f, _sz, _c_f, _sz, _c_f, _sz, _c_f, _c_f, _sz, _u, _c_f]),
}

# include/curl_hip_ragged_msssim.h: the MS-SSIM statistics of a ragged byte batch (a ninth table, for the same reason; the plan
# functions and the workspace query take and fill HOST memory and make no HIP call)
SIGNATURES_RAGGED_MSSSIM = {
    "curl_msssim_ragged_plan_bytes": (_sz, [_i]),
    "curl_msssim_ragged_plan": (_i, [_i, _c_f, _c_f, _i, _c_f, _sz]),
    "curl_msssim_ragged_workspace_bytes": (_sz, [_c_f]),
    "curl_msssim_ragged_u8hwc": (_i, [_c_f, _sz, _c_f, _sz, _c_f, _sz, _c_f, _sz, _c_f, _sz, _c_f, _c_f, _sz, _i, _u, _c_f]),
}
# the plan's layout (int32 words): CURL_MSSSIM_RAGGED_STAMP, _HEADER_WORDS, _DESC_WORDS, _LEVEL_WORD, _LEVEL_WORDS
MSSSIM_RAGGED_STAMP, MSSSIM_RAGGED_HEADER_WORDS, MSSSIM_RAGGED_DESC_WORDS, MSSSIM_RAGGED_LEVEL_WORD, MSSSIM_RAGGED_LEVEL_WORDS = \
    0x4D535231, 32, 64, 16, 8

# include/curl_hip_ragged_loss.h: the CURLLoss statistics of a ragged byte batch (a tenth table, for the same reason; the
# argument lists are the MS-SSIM entries')
SIGNATURES_RAGGED_LOSS = {
    "curl_loss_ragged_plan_bytes": (_sz, [_i]),
    "curl_loss_ragged_plan": (_i, [_i, _c_f, _c_f, _i, _c_f, _sz]),
    "curl_loss_ragged_workspace_bytes": (_sz, [_c_f]),
    "curl_loss_ragged_u8hwc": (_i, [_c_f, _sz, _c_f, _sz, _c_f, _sz, _c_f, _sz, _c_f, _sz, _c_f, _c_f, _sz, _i, _u, _c_f]),
}
# the plan's layout (int32 words): CURL_LOSS_RAGGED_STAMP, _OP, _HEADER_WORDS, _DESC_WORDS, _LEVEL_WORD, _LEVEL_WORDS,
# _TERMS_WORD, _TERMS
LOSS_RAGGED_STAMP, LOSS_RAGGED_OP, LOSS_RAGGED_HEADER_WORDS, LOSS_RAGGED_DESC_WORDS, LOSS_RAGGED_LEVEL_WORD, \
    LOSS_RAGGED_LEVEL_WORDS, LOSS_RAGGED_TERMS_WORD, LOSS_RAGGED_TERMS = 0x4C535231, 6, 32, 64, 16, 8, 28, 5

_lib = None


class CurlHipError(RuntimeError):
    """A HIP runtime error reported by libcurlhip.so (positive return code)."""


def load():
    """Load libcurlhip.so once.  Raises ImportError (never falls back) if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own libamdhip64.so.7; it must be the HIP runtime of the process, so that the
    # device pointers and streams torch hands us belong to the runtime our kernels are launched on.  Loading
    # this library first would bind /opt/rocm's copy instead (observed: hipErrorNoDevice at the first launch).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"curl_amd: HIP library not found at {LIB_PATH}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback for this path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(SIGNATURES_GRAD.items()) + list(SIGNATURES_VIEW.items()) + \
            list(SIGNATURES_FG.items()) + list(SIGNATURES_RAGGED.items()) + list(SIGNATURES_VIEW_RAGGED.items()) + \
            list(SIGNATURES_RAGGED_FG.items()) + list(SIGNATURES_RAGGED_SCORE.items()) + list(SIGNATURES_RAGGED_MSSSIM.items()) + \
            list(SIGNATURES_RAGGED_LOSS.items()):
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


_fast = None
# the entry points csrc/fastcall.cpp calls (their addresses in the library load() bound: CURL_HIP_LIB may name a variant)
FASTCALL_ABI = ("curl_layer_fwd_f32", "curl_layer_bwd_f32", "curl_trispace_fwd_u8hwc", "curl_workspace_bytes",
                "curl_layer_bwd_scratch_bytes")


def fast():
    """The compiled binding of the three hot entry points (curl_amd/_fastcall.*.so, csrc/fastcall.cpp), bound to the library
    load() loaded.  It is part of the build (__graft_entry__.build() asserts it loads); a tree without it warns once and uses
    the ctypes surface -- the same kernels.  CURL_NO_FASTCALL=1 selects the ctypes surface for every call (the A/B of the two
    host paths, tools/small_batch.py)."""
    global _fast
    if _fast is not None:
        return _fast or None
    if os.environ.get("CURL_NO_FASTCALL", "0") == "1":
        _fast = False
        return None
    lib = load()  # the kernels' library: absent -> ImportError, no way around it
    try:
        from . import _fastcall
    except ImportError as e:
        # The binding is host code over the SAME library: without it every call takes the ctypes surface (same kernels, same
        # results, ~10 us more host time per call).  Said once, loudly; tests/test_abi.py and tests/test_gpu_fastcall.py fail on it.
        import warnings
        warnings.warn(f"curl_amd: the compiled binding curl_amd/_fastcall.*.so is missing or does not load ({e}); calls go "
                      "through ctypes. Build it with `python -m curl_amd.build` (g++, a torch C++ extension).", RuntimeWarning)
        _fast = False
        return None
    _fastcall.bind_abi({n: ctypes.cast(getattr(lib, n), ctypes.c_void_p).value for n in FASTCALL_ABI})
    _fast = _fastcall
    return _fast


def check(rc, what):
    """Translate a C-ABI return code into the Python exception the reference's callers would see:
    argument errors -> ValueError (torch raises on bad shapes), HIP errors -> CurlHipError."""
    if rc == 0:
        return
    msg = load().curl_last_error().decode("utf-8", "replace")
    if rc < 0:
        raise ValueError(f"{what}: {msg} (code {rc})")
    raise CurlHipError(f"{what}: {msg} (hipError {rc})")
