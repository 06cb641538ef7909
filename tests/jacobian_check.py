"""What "right" means for the backward of a per-pixel 3 -> 3 operator f(x; knots, mask), Jacobian by pixel -- shared by
tests/test_jacobian_check.py (the host twin, the mutants), tests/test_gpu_pixel_jacobians.py and tests/test_gpu_stage_grads.py
(a plain module like criterion_check.py, not a conftest).  Everything here comes from curl_oracle alone.

Three one-hot cotangents (e_c on every pixel) give row c of every pixel's 3 x 3 Jacobian in one backward call:
  J64 [3,B,3,H,W]  float64 autograd through the oracle at the float32 inputs;  J32 the same in float32 on the CPU
  K64, K32 [3,B,n] the knot Jacobians (row c: d sum_px out_c / d raw)
  mag(px)  |J64[px]|_inf over the nine entries;  G = max mag;  own(px) = max(mag, 1e-3 G)
  C(px)    the curvature, curl_oracle.gradient_curvature's definition for a general f: max over the three channels and both
           signs of |J64(x +- h e_k) - J64(x)|_inf / h, h = 1e-6; for the two stages also with respect to their intermediate
           (the mask times 1 +- h: what the second converter sees of the first one's roundings)
Classes of pixel:
  smooth        1e-6 C <= 1e-3 own  (the project's jump criterion, relative to the pixel's own scale)
  decided kink  not smooth, and for every k and sign J64(x +- eps e_k), eps = 1e-12, agrees with J64(x +- h e_k) within
                1e-3 own: every kink within h is exactly AT the input (a tie, a bound reached exactly, a zero) -- the
                derivative there is a convention, the same in every precision, and a kernel must reproduce it
  near kink     the rest: a kink lies strictly inside (0, h) of the input; either side is float32's to take.  Also a pixel
                whose float64 steps are smooth while the reference's own float32 (at x or a float32 neighbour) is off by more
                than a jump: an intermediate's rounding lands on a kink
tol(px) = REL max(own, C) on smooth pixels, REL max(own, C_side) elsewhere: C is the kink's own there and says nothing about
conditioning, so the curvature is taken BESIDE the kink, C_side = max |J64(x +- 2h e_k) - J64(x +- h e_k)|_inf / h (with REL own
alone the reference's own float32 misses its float64 by 29 tol on the Lab stage's atlas, at a dark pixel of gain 78).
A smooth or decided pixel passes within tol of J64 -- where |J32 - J64| > tol, of J64 or of J32; a near-kink pixel within tol
of any of J64(x), J32(x), the six J64(x +- h e_k) and the six J32(x +- 1 ulp e_k); a candidate other than J64(x) is held
relative to its own magnitude where that is the larger (Reference.errors).  The last six name one class of disagreement: a
float32 evaluation can round its way ONTO a kink that lies within an ulp of the input, and there the convention AT the
kink holds, which is neither side's derivative -- hsv2rgb one ulp below float32(1/6): the kernels' ramps 2 - |6 h - c| have 6 h - 3 round to exactly -2 and pass both ramps' gradients, as
torch.clamp does at a bound and as the reference's own float32 does one ulp further, where 360 h rounds to exactly 60.  A
masked-out pixel of a bool / uint8 mask must be exactly 0.  A non-finite J64 or J32 is refused in the inputs (asserted).
REL is measured, not chosen: max(2e-6, 4 r32), 2e-6 the fused layer's figure (tests/test_gpu_backward.py) and r32 the
reference's own max |J32 - J64| / max(own, C) over the smooth pixels; the factor 4 is criterion_check.MsssimReference's (two
float32 evaluations with different operation orders).  It is never taken from the code under test.
Knot Jacobians are judged on inputs without near-kink pixels, relative to max |K64|: max(2e-5, 4 |K32 - K64| / max |K64|)."""
import itertools

import numpy as np
import torch

import curl_oracle as O

H_STEP = 1e-6      # the curvature's step (curl_oracle.gradient_curvature's)
EPS_STEP = 1e-12   # "exactly at the input"
JUMP = 1e-3        # of own(px)
REL_FLOOR = 2e-6   # tests/test_gpu_backward.py's per-pixel figure
KNOT_FLOOR = 2e-5  # ... and its knot figure at sigma 0.1
FACTOR32 = 4.0     # criterion_check.MsssimReference's
REL_CAP = 1e-4     # an input whose own REL is beyond this is refused
DECIDED_TOL_CAP = 1e-2  # of own(px): a decided kink's tolerance beyond this is refused as an input (Reference.__init__)
INFLATION_NOTED = 10.0  # decided kinks judged more than this many times looser than REL own are counted in every report

CONVERTERS = ("rgb2lab", "lab2rgb", "rgb2hsv", "hsv2rgb")
CURVE_OPS = {"adjust_rgb": 3, "adjust_lab": 3, "adjust_hsv": 4, "lab_stage": 3, "hsv_stage": 4}
STAGES = ("lab_stage", "hsv_stage")
# the device tests' shapes: HW = 1172 = 4 x 293 (the float4 kernels: two 256-lane blocks, the second ragged) and an odd HW (the
# scalar kernels)
SHAPES = {"float4": (2, 4, 293), "scalar": (1, 37, 53)}
# a colour at which the operator is smooth (no tie, no bound, no threshold nearby): what near-kink pixels are replaced by
SMOOTH_COLOUR = {"lab2rgb": (0.6, 0.5, 0.55), "hsv2rgb": (0.3, 0.5, 0.6), "adjust_hsv": (0.3, 0.5, 0.6), "adjust_lab": (0.6, 0.5, 0.55)}
SMOOTH_RGB = (0.6, 0.4, 0.25)


def oracle_forward(op, x, raw=None, mask=None):
    """out [B,3,H,W] of the oracle's `op` in x's dtype (mask: None = ones, as the reference's stages take it)."""
    if op in CONVERTERS:
        return getattr(O, op)(x)
    if op in STAGES:
        m = torch.ones_like(x[:, :1]) if mask is None else mask.to(x.dtype)
        return getattr(O, op)(x, m, raw, raw.shape[1])[0]
    return getattr(O, op)(x, raw)[0]


def oracle_jacobians(op, xs, raw=None, mask=None, mask_factors=None):
    """xs: a list of V inputs [B,3,H,W] of one dtype -> (J [V,3,B,3,H,W], K [V,3,B,n] or None): the three one-hot
    cotangents of every input ride in one batch (every operator here is per pixel, and knots are per image).
    mask_factors: per input, a factor on the mask (the stages' intermediate, perturbed)."""
    V, (B, _, H, W) = len(xs), xs[0].shape
    dt = xs[0].dtype
    X = torch.cat([x for x in xs for _ in range(3)], 0).detach().clone().requires_grad_(True)
    rep = 3 * V
    k = None if raw is None else raw.to(dt).repeat(rep, 1).requires_grad_(True)
    m = None if mask is None else mask.to(dt).reshape(-1, 1, H, W).expand(B, 1, H, W).repeat(rep, 1, 1, 1)
    if mask_factors is not None:
        m = torch.ones(rep * B, 1, H, W, dtype=dt) if m is None else m
        m = m * torch.tensor(mask_factors, dtype=dt).repeat_interleave(3 * B).reshape(-1, 1, 1, 1)
    out = oracle_forward(op, X, k, m)
    w = torch.zeros(V, 3, B, 3, H, W, dtype=dt)
    for c in range(3):
        w[:, c, :, c] = 1
    g = torch.autograd.grad((out * w.reshape(out.shape)).sum(), [X] if k is None else [X, k])
    return g[0].reshape(V, 3, B, 3, H, W).double(), None if k is None else g[1].reshape(V, 3, B, -1).double()


def _px(t):
    """|t|_inf over the Jacobian's nine entries: [..., 3, B, 3, H, W] -> [..., B, H, W]."""
    return t.abs().amax(-3).amax(-4)


class Reference:
    """J64, J32, the perturbed Jacobians and everything derived from them alone, for `op` at the float32 input x."""

    def __init__(self, op, x, raw=None, mask=None, label=""):
        assert x.dtype == torch.float32
        self.op, self.label = op, label or op
        self.x = x.detach().cpu()
        self.raw = None if raw is None else raw.detach().cpu().float()
        self.mask = None if mask is None else mask.detach().cpu()
        x64 = self.x.double()
        steps = [(k, s * d) for d in (H_STEP, EPS_STEP, 2 * H_STEP) for k in range(3) for s in (1.0, -1.0)]
        xs = [x64]
        for k, d in steps:
            p = x64.clone()
            p[:, k] += d
            xs.append(p)
        raw64 = None if self.raw is None else self.raw.double()
        factors = None
        if op in STAGES:  # the mask multiplies the stage's intermediate (Lab, HSV): +-1e-6 of it, relative
            xs += [x64, x64]
            factors = [1.0] * 19 + [1.0 + H_STEP, 1.0 - H_STEP]
        J, K = oracle_jacobians(op, xs, raw64, self.mask, factors)
        self.J64, self.Jh, Je, J2h = J[0], J[1:7], J[7:13], J[13:19]
        self.K64 = None if K is None else K[0]
        xs32 = [self.x]
        for k in range(3):
            for towards in (float("inf"), -float("inf")):
                p = self.x.clone()
                p[:, k] = torch.nextafter(p[:, k], torch.tensor(towards))
                xs32.append(p)
        J32, K32 = oracle_jacobians(op, xs32, self.raw, self.mask)
        self.J32, self.J32n, self.K32 = J32[0], J32[1:], None if K32 is None else K32[0]
        # a non-finite reference is a fault of the inputs: never left out of the comparison, refused here
        assert bool(torch.isfinite(J).all()) and bool(torch.isfinite(J32).all()), f"{self.label}: non-finite reference Jacobian"
        self.mag = _px(self.J64)
        self.G = float(self.mag.max())
        self.own = self.mag.clamp(min=1e-3 * self.G)
        self.C = _px(self.Jh - self.J64).amax(0) / H_STEP
        self.smooth = H_STEP * self.C <= JUMP * self.own
        self.decided = ~self.smooth & (_px(Je - self.Jh).amax(0) <= JUMP * self.own)
        self.near = ~self.smooth & ~self.decided
        # ... and a pixel the float64 steps call smooth while the reference's own float32, at x or at one of its six float32
        # neighbours, is off by more than a jump: a rounding of some INTERMEDIATE lands on or across a kink that no input
        # step of h reaches (a curve's product rounding to exactly 1.0, the clamp's bound, where float64 has 1 + 1e-8).  Rare:
        # 8 and 12 pixels of the HSV stage's atlas under a bool / soft mask with the uneven 61-knot split, none elsewhere
        # (n_two_minds is printed with every case); without it those pixels made r32 470 and REL meaningless
        two_minds = self.smooth & (_px(J32 - self.J64).amax(0) > JUMP * self.own)
        self.smooth, self.near = self.smooth & ~two_minds, self.near | two_minds
        self.n_two_minds = int(two_minds.sum())
        self.scale = torch.maximum(self.own, self.C)
        # beside the kink: the curvature one step further out, where the step from x +- h to x +- 2h crosses nothing
        self.C_side = _px(J2h - self.Jh).amax(0) / H_STEP
        # a stage's second converter sees its first one's roundings: the curvature with respect to the intermediate, which
        # the input's cannot show where the curves between them are clamped flat (an out-of-gamut colour with L and a curve-
        # saturated: XYZ -> RGB cancels to 1 % of its terms, and float32 loses 1e-5 of d gamma / d v whoever evaluates it)
        self.C_mid = _px(J[19:21] - self.J64).amax(0) / H_STEP if op in STAGES else torch.zeros_like(self.C)
        self.scale = torch.maximum(self.scale, self.C_mid)
        d32 = _px(self.J32 - self.J64)
        self.r32 = float((d32 / self.scale.clamp(min=1e-300))[self.smooth].max()) if bool(self.smooth.any()) else 0.0
        self._d32 = d32
        self.set_rel(max(REL_FLOOR, FACTOR32 * self.r32))
        # a condition on the inputs: beyond half of the bar this protocol replaces (2e-4 of the tensor-wide maximum) the
        # reference's own float32 says the input cannot judge anything
        assert self.rel <= REL_CAP, f"{self.label}: REL = {self.rel:.2e} from the reference's own float32: choose other inputs"
        # ... and so is a decided kink judged too loosely to tell a convention from its alternative.  C_side (and C_mid) stand
        # in for the conditioning the kink hides -- a tie of two 8-bit neighbours has d hue / d x ~ 1 / (6 df) and a curvature of
        # 2 / df = 510 times that, tol = 1e-3 own at REL 2e-6 -- but the other convention moves an entry by about own itself (a
        # gate's whole gradient, a tie's one-hot): 1 % of own keeps a margin of a hundred.  The inflation is printed with every
        # case (report); the assertion is set_rel's.
        self.dead = None
        if self.mask is not None and self.mask.dtype in (torch.bool, torch.uint8):
            B, _, H, W = self.x.shape
            self.dead = (self.mask.reshape(-1, H, W) == 0).expand(B, H, W)

    def set_rel(self, rel):
        """REL and what follows from it.  (An atlas is ONE content judged in parts: its parts share the REL of their largest
        r32, share_rel.)"""
        self.rel = rel
        self.tol = rel * torch.where(self.smooth, self.scale, torch.maximum(torch.maximum(self.own, self.C_side), self.C_mid))
        self.ambiguous = self._d32 > self.tol
        worst = float((self.tol / self.own.clamp(min=1e-300))[self.decided].max()) if bool(self.decided.any()) else 0.0
        assert worst <= DECIDED_TOL_CAP, f"{self.label}: a decided kink is judged to {worst:.2e} of its own scale: choose other inputs"

    def inflation(self, cls="decided"):
        """max over the decided-kink (or near-kink) pixels of tol / (REL own): what C_side and C_mid add to the bare REL own
        there.  Reported with every case (report) so that a pixel judged loosely stays visible."""
        sel = self.decided if cls == "decided" else self.near
        return float((self.tol / (self.rel * self.own).clamp(min=1e-300))[sel].max()) if bool(sel.any()) else 1.0

    def decided_beyond(self, factor=INFLATION_NOTED):
        """How many decided-kink pixels are judged more than `factor` times looser than REL own."""
        return int((self.decided & (self.tol > factor * self.rel * self.own)).sum())

    # ---- the classes, as figures for a table
    def counts(self):
        return {"smooth": int(self.smooth.sum()), "decided": int(self.decided.sum()), "near": int(self.near.sum())}

    def cls(self, b, y, x):
        return "smooth" if self.smooth[b, y, x] else "decided kink" if self.decided[b, y, x] else "near kink"

    def describe(self, got, b, y, x):
        f = lambda t: np.array2string(t[:, b, :, y, x].numpy(), precision=9, separator=",").replace("\n", "")  # noqa: E731
        return (f"{self.label} pixel (b={b}, y={y}, x={x}): input={[float(v) for v in self.x[b, :, y, x]]} class={self.cls(b, y, x)}"
                f"{'' if self.mask is None else ' mask=' + str(float(self.mask.reshape(-1, *self.x.shape[2:])[b % self.mask.shape[0], y, x]))}\n"
                f"  got={f(got)}\n  J64={f(self.J64)}\n  J32={f(self.J32)}\n"
                f"  tol={float(self.tol[b, y, x]):.3e} own={float(self.own[b, y, x]):.3e} C={float(self.C[b, y, x]):.3e} "
                f"G={self.G:.3e} REL={self.rel:.3e} (r32={self.r32:.3e})")

    def errors(self, got):
        """-> got as float64, and per pixel [B,H,W] min over the protocol's candidates of |got - candidate|_inf / tol.  A
        candidate other than J64 is held relative to ITS OWN magnitude where that is the larger: tol max(1, |candidate|_inf / own)
        -- across a kink the other side can be orders above own(px) (a closed gate's 0 beside an open one's 2), and float32
        reaches a value to REL of that value, no closer.  (NaN counts as inf.)"""
        got = got.detach().double().cpu()
        assert got.shape == self.J64.shape, (got.shape, self.J64.shape)

        def ratio(cand):
            d = _px(got - cand)
            d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
            return d / (self.tol * torch.clamp(_px(cand) / self.own, min=1.0)).clamp(min=1e-300)
        r64 = _px(got - self.J64)
        r64 = torch.where(torch.isnan(r64), torch.full_like(r64, float("inf")), r64) / self.tol.clamp(min=1e-300)
        r32 = ratio(self.J32)
        err = torch.where(self.ambiguous, torch.minimum(r64, r32), r64)
        if bool(self.near.any()):
            cand = torch.minimum(torch.minimum(r64, r32), torch.minimum(ratio(self.Jh).amin(0), ratio(self.J32n).amin(0)))
            err = torch.where(self.near, cand, err)
        return got, err

    def worst(self, got):
        """max over the smooth pixels of |got - J64|_inf / max(own, C): the figure DESIGN.md tabulates."""
        got = got.detach().double().cpu()
        r = _px(got - self.J64) / self.scale.clamp(min=1e-300)
        return float(r[self.smooth].max()) if bool(self.smooth.any()) else 0.0

    def check(self, got):
        """Assert the Jacobian `got` [3,B,3,H,W] against the protocol; on failure the message names the worst pixel.
        -> worst(got)."""
        got, err = self.errors(got)
        if self.dead is not None:
            bad = self.dead & (got != 0).any(0).any(1)  # (NaN != 0: a NaN under the mask fails here)
            if bool(bad.any()):
                b, y, x = (int(v) for v in bad.nonzero()[0])
                raise AssertionError(f"masked-out pixel is not exactly 0 ({int(bad.sum())} such)\n" + self.describe(got, b, y, x))
        over = ~(err <= 1.0)
        if bool(over.any()):
            ratio = torch.where(over, err, torch.zeros_like(err))
            b, y, x = (int(v) for v in (ratio == ratio.max()).nonzero()[0])
            raise AssertionError(f"{int(over.sum())} pixels beyond tol(px); the worst is {float(ratio.max()):.3g} x tol\n"
                                 + self.describe(got, b, y, x))
        return self.worst(got)

    def knot_bound(self):
        scale = max(float(self.K64.abs().max()), 1e-300)
        return max(KNOT_FLOOR, FACTOR32 * float((self.K32 - self.K64).abs().max()) / scale), scale

    def check_knots(self, got):
        """Assert the knot Jacobian `got` [3,B,n]; only on inputs without near-kink pixels. -> the relative error."""
        assert int(self.near.sum()) == 0, f"{self.label}: knot Jacobians are judged on inputs without near-kink pixels"
        got = got.detach().double().cpu()
        assert got.shape == self.K64.shape, (got.shape, self.K64.shape)
        bound, scale = self.knot_bound()
        r = float((got - self.K64).abs().max()) / scale
        assert r <= bound, f"{self.label}: knot Jacobian off by {r:.3e} of its scale {scale:.3e}; the bound is {bound:.3e}"
        return r


def share_rel(refs):
    """The parts of one atlas take the REL of the largest r32 among them."""
    rel = max(r.rel for r in refs)
    for r in refs:
        r.set_rel(rel)
    return refs


def smooth_colour(op):
    return torch.tensor(SMOOTH_COLOUR.get(op, SMOOTH_RGB), dtype=torch.float32).reshape(1, 3, 1, 1)


def decidable_inputs(op, x, raw=None, mask=None, label="", max_share=0.01):
    """Input hygiene for content inputs: near-kink pixels are replaced IN THE INPUTS by a colour that is smooth for `op`
    (never left out of the comparison); at most max_share of the pixels (None: any share -- an atlas being prepared for its
    knot check); none remains.  Decided kinks stay in.  -> the Reference of the cleaned input (its .x is the input to use)."""
    ref = Reference(op, x, raw, mask, label)
    n = int(ref.near.sum())
    if n == 0:
        return ref
    assert max_share is None or n <= max_share * ref.near.numel(), f"{label}: {n} of {ref.near.numel()} pixels are near a kink (> {max_share:.0%})"
    ref = Reference(op, torch.where(ref.near[:, None], smooth_colour(op), ref.x), raw, mask, label)
    assert int(ref.near.sum()) == 0, f"{label}: {int(ref.near.sum())} near-kink pixels remain after the replacement"
    return ref


# ------------------------------------------------------------------------------------------------------------------
# contents and edge atlases (built in float64, rounded to float32)
# ------------------------------------------------------------------------------------------------------------------
def f32(v):
    return float(np.float32(v))


def ulp(v, k):
    """The float32 k steps from float32(v)."""
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return float(v)


def _product(c0, c1, c2, op):
    """The Cartesian product of three value lists as [1,3,4,N/4] float32, padded with the operator's smooth colour."""
    px = np.array(list(itertools.product(c0, c1, c2)), np.float64)
    pad = (-len(px)) % 4
    px = np.concatenate([px, np.tile(np.array(SMOOTH_COLOUR.get(op, SMOOTH_RGB), np.float64), (pad, 1))])
    return torch.from_numpy(px.astype(np.float32).T.copy()).reshape(1, 3, 4, -1).contiguous()


def grey_at_cie_threshold():
    """The grey value at which Y (= the linearised value: the Y row sums to 1) crosses (6/29)^3."""
    return 1.055 * ((6.0 / 29.0) ** 3) ** (1.0 / 2.4) - 0.055


def atlas(op):
    """The edge atlas of `op`'s input space: a list of (part, [1,3,4,N/4] float32).  Each part is judged as an input of its
    own, with its own G: two values one ulp apart in two channels are, for rgb2hsv, a hue gradient of 1 / (6 ulp) ~ 1e7, and
    own(px) >= 1e-3 G would put every other pixel of the same input out of sight.  So the values that are ulps from each other
    (part "ulps") are kept apart from the bounds, floors and exact ties (part "edges")."""
    if op == "lab2rgb":
        L = [ulp(0.08, k) for k in (-1, 0, 1)] + [0.0, 1.0, 1.05, -0.02]  # fy = (100 L + 16) / 116 = 6/29 at L = 0.08
        ab = [0.0, 0.25, 0.45, 0.5, 0.55, 0.75, 1.0]  # out-of-gamut (negative v) and v about the linear threshold among them
        return [("edges", _product(L, ab, ab, op))]
    if op in ("hsv2rgb", "adjust_hsv"):
        h = [0.0, 1e-9, 0.5, 1.0, 1.1, -0.1] + [ulp(k / 6.0, d) for k in (1, 2, 4, 5) for d in (-1, 0, 1)]
        sv = [0.0, 1e-9, 0.3, 1.0, 1.2, -0.1]
        return [("edges", _product(h, sv, sv, op))]
    thr, grey = 0.04045, grey_at_cie_threshold()
    e = [0.0, 0.5e-9, 1e-9, 1.0 / 255, 1.0, 1.001, -0.01, f32(thr), f32(grey), 0.2, 0.5]
    # (0.04045's +-2 ulp neighbours are left out: with them more than half of rgb2lab's atlas is near a kink)
    u = [ulp(thr, k) for k in (-1, 0, 1)] + [ulp(grey, k) for k in (-1, 0, 1)] + [0.2, ulp(0.2, 1)]
    return [("edges", _product(e, e, e, op)), ("ulps", _product(u, u, u, op))]


# operators whose reference has convention points a float32 input can hit exactly (a tie, a clamp bound, a floor).  rgb2lab and
# lab2rgb have none: their only branches are thresholds no float32 value equals (0.04045, (6/29)^3 and 6/29 of COMPUTED values,
# 0.0031308), and the Lab stage's curves meet a bound exactly only at black -- their atlases hold smooth and near-kink pixels.
HAS_CONVENTION_POINTS = ("rgb2hsv", "hsv2rgb", "adjust_rgb", "adjust_lab", "adjust_hsv", "hsv_stage")


def atlas_conditions(op, refs, decided=True):
    """The conditions on an atlas, from the oracle alone (the References of its parts): no non-finite pixel (Reference asserts
    it), at least 100 smooth pixels, at least 100 decided kinks where the operator has any, a near-kink share below one half."""
    n = {k: sum(r.counts()[k] for r in refs) for k in ("smooth", "decided", "near")}
    total = sum(n.values())
    assert n["smooth"] >= 100, (op, n)
    assert n["decided"] >= 100 or not decided or op not in HAS_CONVENTION_POINTS, (op, n)
    assert n["near"] < 0.5 * total, (op, n)
    return n


# operators that begin with rgb2hsv: an exact 0 lies 1e-9 below its floor (colors.py:205), a kink strictly inside (0, h)
FLOOR_BELOW_ZERO = ("rgb2hsv", "hsv_stage")


def content(kind, op, shape, seed):
    """random / wide (the operator's range overshot: rand * 1.1 - 0.04) / grid8: the k/255 grid, k = 0 .. 255, with the first
    third of the rows tied (channel 1 = channel 0).  For the operators that begin with rgb2hsv k starts at 1: there an exact
    0 is a near kink (FLOOR_BELOW_ZERO) on more than 1 % of an 8-bit image's pixels, and is the atlas's to meet; for every
    other operator an exact 0 is smooth or a decided kink and stays in."""
    g = torch.Generator().manual_seed(seed)
    B, H, W = shape
    if kind == "grid8":
        img = torch.randint(1 if op in FLOOR_BELOW_ZERO else 0, 256, (B, 3, H, W), generator=g).float() / 255
        img[:, 1, : max(1, H // 3)] = img[:, 0, : max(1, H // 3)]
        return img
    img = torch.rand(B, 3, H, W, generator=g)
    return img * 1.1 - 0.04 if kind == "wide" else img


def knots(op, kind, B, seed, n=None):
    """Raw knots [B,n]: s01 / s03 (sigma 0.1 / 0.3) or 'sat' (sigma 0.3 shifted by +0.5: the curves' output clamps close)."""
    g = torch.Generator().manual_seed(seed)
    n = n or 16 * CURVE_OPS[op]
    raw = torch.randn(B, n, generator=g)
    return raw * 0.1 if kind == "s01" else raw * 0.3 if kind == "s03" else raw * 0.3 + 0.5


def one_hot_jacobian(fn, shape):
    """got [3,B,3,H,W] (and K [3,B,n] where fn returns a pair) from three calls fn(grad_out) with one-hot grad_out."""
    B, H, W = shape
    rows, krows = [], []
    for c in range(3):
        go = torch.zeros(B, 3, H, W)
        go[:, c] = 1
        r = fn(go)
        if isinstance(r, tuple):
            krows.append(r[1])
            r = r[0]
        rows.append(r)
    J = None if rows[0] is None else torch.stack([torch.as_tensor(r) for r in rows])
    return (J, torch.stack([torch.as_tensor(k) for k in krows])) if krows else J


# ------------------------------------------------------------------------------------------------------------------
# the cases, shared by the host-twin and the device tests (each Reference is built once and left unchanged)
# ------------------------------------------------------------------------------------------------------------------
CONTENTS = ("random", "wide", "grid8", "atlas")
KNOT_KINDS = ("s01", "s03", "sat")  # every content and the atlas meet all three
MASKS = ("none", "bool", "uint8", "soft", "bool_mask_first")
_REFS = {}


def knot_kinds(op, kind):
    return KNOT_KINDS if op in CURVE_OPS else (None,)


def make_mask(mask_kind, x):
    """none / bool with the first 256 pixels of image 0 off (a whole 256-lane block and its waves dead) and a fifth of the
    rest / the same as uint8 / a soft float mask in (0, 1) / the bool one again (the caller adds F_MASK_FIRST)."""
    if mask_kind == "none":
        return None
    B, _, H, W = x.shape
    g = torch.Generator().manual_seed(5)
    u = torch.rand(B, 1, H, W, generator=g)
    if mask_kind == "soft":
        return u * 0.98 + 0.01
    m = u > 0.2
    m.view(B, -1)[0, :256] = False
    return m.to(torch.uint8) if mask_kind == "uint8" else m


def case_references(op, kind, kk, shape=None, mask_kind="none", n=None, seed=3):
    """The References of one case -- the cleaned content at `shape`, or the atlas's parts -- with the input conditions asserted
    from the oracle alone: a content has at most 1 % of its pixels replaced and no near-kink pixel left; an atlas is finite,
    holds >= 100 smooth and (where the operator has convention points; under the wider knots most of the HSV stage's atlas is
    clamped flat, and the count is the sigma-0.1 run's to meet) >= 100 decided-kink pixels and is less than half near-kink."""
    mask_kind = "bool" if mask_kind == "bool_mask_first" else mask_kind  # (the same mask; the caller adds the flag)
    key = (op, kind, kk, shape if kind != "atlas" else None, mask_kind, n, seed)
    if key not in _REFS:
        if kind == "atlas":
            refs = []
            for part, x in atlas(op):
                raw = None if kk is None else knots(op, kk, 1, 11, n)
                refs.append(Reference(op, x, raw, make_mask(mask_kind, x), f"{op} atlas/{part} {kk or ''} {mask_kind}"))
            atlas_conditions(op, refs, decided=kk in (None, "s01") and mask_kind == "none")
            _REFS[key] = share_rel(refs)
        else:
            x = content(kind, op, shape, seed)
            raw = None if kk is None else knots(op, kk, shape[0], 11, n)
            _REFS[key] = [decidable_inputs(op, x, raw, make_mask(mask_kind, x), f"{op} {kind} {kk or ''} {mask_kind} {shape}")]
    return _REFS[key]


def knot_reference(ref):
    """The Reference on which `ref`'s knot Jacobian is judged: ref itself, or -- an atlas part with near-kink pixels -- the
    part with those pixels replaced by the smooth colour (any share of them)."""
    if int(ref.near.sum()) == 0:
        return ref
    key = ("knots", ref.label)
    if key not in _REFS:
        _REFS[key] = decidable_inputs(ref.op, ref.x, ref.raw, ref.mask, ref.label + " cleaned", max_share=None)
    return _REFS[key]


def reg_knot_reference(op, raw):
    """d reg_b / d raw_b in float64 and float32 [B,n] (the regulariser sees the knots alone)."""
    out = []
    for dt in (torch.float64, torch.float32):
        k = raw.to(dt).clone().requires_grad_(True)
        x = torch.full((raw.shape[0], 3, 1, 1), 0.5, dtype=dt)
        reg = getattr(O, op)(x, torch.ones_like(x[:, :1]), k, k.shape[1])[1] if op in STAGES else getattr(O, op)(x, k)[1]
        out.append(torch.autograd.grad(reg.sum(), k)[0].double())
    return out


def report(ref, figure, who):
    """One line for the record (DESIGN.md's table is filled from these)."""
    c = ref.counts()
    return (f"jacobian | {ref.label} | r32 {ref.r32:.1e} | {who} {figure:.1e} | REL {ref.rel:.1e} | "
            f"{c['smooth']} / {c['decided']} / {c['near']} | infl {ref.inflation():.3g} ({ref.decided_beyond()} px) "
            f"near {ref.inflation('near'):.3g} two-minds {ref.n_two_minds}")
