"""Polynomial orders 1-3 of the polynomial layers and TriSpaceRegNet, without a GPU: the Python surface, the C ABI's argument
checks, the host twin of the per-order Horner schemes, the generated tables, the padding rule of the backward, and the
composed oracle (tests/poly_orders_ref.py) against outputs of the reference's own classes (tests/golden/poly_orders.npz)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import curl_oracle as O
import poly_orders_ref as R
from conftest import ROOT, max_err
from twin_build import FLAVOURS, twin_library

E_NULL, E_SHAPE, E_KNOTS = -1, -2, -3


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _small_backbone():
    from curl_amd import model
    return model.CurveEncoder(num_outputs=1, num_features=64, width=0.25)


# ------------------------------------------------------------------ the Python surface
@pytest.mark.parametrize("spatial", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_trispace_regnet_constructs_with_the_reference_state(golden, d, spatial):
    """TriSpaceRegNet(polynomial_order=d, spatial=s): num_coeffs = n(d, V), and the state a reference checkpoint of the same
    arguments holds -- `polylayer.powers` [n, V] as the reference's generate_powers lists them, the head's last layer
    [9 n, 512], the coordinate ramps, the colour constants -- key for key and shape for shape; it loads strict."""
    from curl_amd import model
    from curl_amd.convert_state import convert_state_dict
    from test_checkpoint_compat import _reference_trispace_checkpoint
    V = 5 if spatial else 3
    n = R.n_coeffs(d, V)
    net = model.TriSpaceRegNet(polynomial_order=d, spatial=spatial)
    assert net.num_coeffs == n and net.order == d
    mine = net.state_dict()
    powers = golden("poly_orders")[f"powers_d{d}_v{V}"]
    assert powers.shape == (n, V) and np.array_equal(mine["polylayer.powers"].numpy().astype(np.int32), powers)
    ckpt = _reference_trispace_checkpoint(spatial)  # the order-4 checkpoint of the reference's constructor (model.py:451-484) ...
    ckpt["module.polylayer.powers"] = torch.from_numpy(powers).float()  # ... with what the order sizes (model.py:212-216, 463)
    ckpt["module.backbone.classifier.3.weight"] = torch.zeros(9 * n, 512)
    ckpt["module.backbone.classifier.3.bias"] = torch.zeros(9 * n)
    for k in list(ckpt):
        if ckpt[k] is None:
            ckpt[k] = mine[k[len("module."):]].clone()
    conv = convert_state_dict(ckpt)
    assert set(conv) == set(mine), (sorted(set(conv) - set(mine))[:5], sorted(set(mine) - set(conv))[:5])
    for k, v in conv.items():
        assert tuple(v.shape) == tuple(mine[k].shape), k
    net.load_state_dict(conv, strict=True)


def test_poly_regnet_and_small_models_size_their_heads_by_the_order():
    from curl_amd import model
    for d in (1, 2, 3, 4):
        p = model.PolyRegNet(polynomial_order=d, backbone=_small_backbone(), feature_width=64)
        assert p.num_coeffs == R.n_coeffs(d, 3) and p.backbone.classifier.out_features == 3 * p.num_coeffs
        for spatial in (False, True):
            n = model.TriSpaceRegNet(polynomial_order=d, spatial=spatial, backbone=_small_backbone(), feature_width=64)
            assert n.num_coeffs == R.n_coeffs(d, 5 if spatial else 3)
            assert n.backbone.classifier[3].out_features == 9 * n.num_coeffs


def test_reference_default_layer_reaches_the_device_check():
    """ChannelPolyLayer() is the reference's default construction (degree 3, 3 variables): on a CPU tensor its forward gets as
    far as "this path runs on a HIP device only", not NotImplementedError."""
    from curl_amd import model
    lay = model.ChannelPolyLayer()
    assert (lay.degree, lay.num_variables, lay.num_out, lay.num_coeffs) == (3, 3, 3, 20)
    with pytest.raises(RuntimeError, match="HIP device only"):
        lay(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 20))
    for d, V in ((1, 5), (2, 5), (3, 5), (1, 3), (2, 3)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            model.ChannelPolyLayer(d, V, 3)(torch.zeros(1, V, 4, 4), torch.zeros(1, 3, R.n_coeffs(d, V)))


@pytest.mark.parametrize("args", [(0, 3, 3), (5, 3, 3), (3, 4, 3), (3, 2, 3), (3, 3, 2), (2, 5, None)])
def test_unbuilt_configurations_still_raise_and_say_what_is_built(args):
    from curl_amd import model
    lay = model.ChannelPolyLayer(*args)
    with pytest.raises(NotImplementedError, match="degree 1 to 4, 3 or 5 variables, 3 outputs"):
        lay(torch.zeros(1, lay.num_variables, 4, 4), torch.zeros(1, lay.num_out, lay.num_coeffs))
    with pytest.raises(NotImplementedError, match="polynomial_order 1 to 4"):
        model.TriSpaceRegNet(polynomial_order=0, backbone=_small_backbone(), feature_width=64)
    with pytest.raises(NotImplementedError, match="polynomial_order 1 to 4"):
        model.TriSpaceRegNet(polynomial_order=5, spatial=True, backbone=_small_backbone(), feature_width=64)


def test_train_and_infer_take_the_order():
    from curl_amd import infer, train
    net = train.build_net("trispace", 0.25, False, polynomial_order=2)
    assert net.order == 2 and net.num_coeffs == 21
    assert train.build_net("trispace", 0.25, False).num_coeffs == 126
    net = infer.build_net("random", torch.device("cpu"), arch="trispace", polynomial_order=3)
    assert net.num_coeffs == 56 and not net.is_train


# ------------------------------------------------------------------ the C ABI, before any HIP call
def test_forward_entries_take_the_new_counts_and_refuse_the_others():
    """Every new count, with its order in the high half (CURL_POLY_COEFFS), passes the num_coeffs check of the three forward
    entries: a table that is not 4-byte aligned is then CURL_E_SHAPE (none of the new kernels copies 8-byte pairs; with fake
    pointers an aligned call would go on to launch, which is not tried here).  Counts between the valid ones, a count under
    another order, and a plain lower-order count -- recorded as CURL_E_KNOTS by tests/data/launch_plan.txt -- are CURL_E_KNOTS."""
    from curl_amd import _lib
    lib = _lib.load()
    assert lib.curl_version() >= 113
    fake, two = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 2)
    PC = _lib.poly_coeffs
    assert PC(56, 3) == 56 | (3 << 16) and PC(56, 0) >> 16 == 0x7fff
    src = open(os.path.join(ROOT, "include", "curl_hip_poly.h")).read()
    assert ("#define CURL_POLY_COEFFS(num_coeffs, order) ((int)((unsigned)(num_coeffs) | ((unsigned)((order) > 0 ? (order) : 0x7fff) << 16)))"
            in src)

    def three(coeffs, nc):
        return (lib.curl_trispace_fwd_f32(fake, coeffs, fake, 1, 8, 8, nc, 0, None),
                lib.curl_trispace_fwd_slab_f32(fake, coeffs, fake, 1, 8, 8, 0, 4, nc, 0, None),
                lib.curl_trispace_fwd_u8hwc(fake, coeffs, None, fake, 1, 8, 8, nc, 0, None))
    for d, _, nc in R.NEW_COUNTS:
        assert three(two, PC(nc, d)) == (E_SHAPE,) * 3, nc
        assert b"4-byte aligned" in lib.curl_last_error()
        assert three(fake, nc) == (E_KNOTS,) * 3, nc                      # the order has to be said
        assert three(fake, PC(nc, d % 3 + 1)) == (E_KNOTS,) * 3, nc       # ... and be the count's own
        assert b"polynomial order" in lib.curl_last_error()
    assert three(two, PC(35, 4)) == (E_SHAPE,) * 3 and b"4-byte aligned" in lib.curl_last_error()
    assert three(ctypes.c_void_p(4096 + 4), PC(126, 4)) == (E_SHAPE,) * 3 and b"8-byte aligned" in lib.curl_last_error()
    for nc in (5, 34, 57, 100, 0, -4, 127):
        assert three(fake, nc) == (E_KNOTS,) * 3, nc
        for d in (0, 1, 2, 3, 4, 5):
            assert three(fake, PC(nc & 0xffff, d)) == (E_KNOTS,) * 3, (nc, d)


def test_poly_layer_takes_the_degree_in_the_high_half():
    from curl_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    PV = _lib.poly_vars
    assert PV(5, 3) == 5 | (3 << 16) and PV(3, 4) >> 16 == 4 and PV(5, 0) >> 16 == 0x7fff
    src = open(os.path.join(ROOT, "include", "curl_hip_poly.h")).read()
    assert "#define CURL_POLY_VARS(V, degree) ((int)((unsigned)(V) | ((unsigned)((degree) > 0 ? (degree) : 0x7fff) << 16)))" in src
    for V in (5, 3):
        for d in (1, 2, 3, 4):
            assert lib.curl_poly_layer_f32(None, fake, fake, 1, 8, 8, PV(V, d), None) == E_NULL  # the image, not the shape
            assert lib.curl_poly_layer_f32(fake, None, fake, 1, 8, 8, PV(V, d), None) == E_NULL
            assert b"coeffs" in lib.curl_last_error()
    for V, d in ((5, 0), (5, 5), (4, 3), (0, 3), (5, -1), (126, 1)):
        assert lib.curl_poly_layer_f32(fake, fake, fake, 1, 8, 8, PV(V, d), None) == E_SHAPE, (V, d)
        assert b"num_variables" in lib.curl_last_error()
    # the backward entry stays degree 4: a packed degree is a shape error there
    assert lib.curl_poly_layer_bwd_f32(fake, fake, fake, fake, fake, fake, 1 << 30, 1, 8, 8, PV(5, 3), 0, None) == E_SHAPE


def test_new_header_compiles_as_c99_and_cxx(tmp_path):
    import shutil
    if not shutil.which("gcc"):
        pytest.skip("gcc not present")
    src = tmp_path / "h.c"
    src.write_text('#include "curl_hip_poly.h"\nint main(void) { return CURL_POLY_VARS(5, 3) == (5 | 3 << 16) && CURL_POLY_VARS(3, 0) != 3 && CURL_POLY_COEFFS(56, 3) == (56 | 3 << 16) ? 0 : 1; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", str(src), "-I", inc, "-o", str(tmp_path / "c")])
    subprocess.check_call([str(tmp_path / "c")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-x", "c++", "-c", str(src), "-I", inc, "-o", str(tmp_path / "cc.o")])


# ------------------------------------------------------------------ Python-side padding of the backward
class _Recorder:
    """Stands in for the loaded library: records what the order-4 backward entries are handed, writes a gradient."""

    def __init__(self):
        self.seen = {}

    def curl_trispace_bwd_scratch_bytes(self, B, H, W, nc):
        return 64

    def _table(self, ptr, n):
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float)), (n,)).copy()

    def curl_trispace_bwd_f32(self, img, c, gout, g, scratch, nbytes, B, H, W, nc, flags, stream):
        self.seen["bwd"] = (nc, self._table(c, B * 9 * nc).reshape(B, 3, 3, nc), c % 8)
        np.ctypeslib.as_array(ctypes.cast(g, ctypes.POINTER(ctypes.c_float)), (B * 9 * nc,))[:] = np.arange(B * 9 * nc)
        return 0

    def curl_trispace_bwd_img_f32(self, img, c, gout, g, B, H, W, nc, flags, stream):
        self.seen["bwd_img"] = (nc, self._table(c, B * 9 * nc).reshape(B, 3, 3, nc), c % 8)
        return 0

    def curl_poly_layer_bwd_scratch_bytes(self, B, H, W, V):
        return 64

    def curl_poly_layer_bwd_f32(self, img, c, gout, gimg, gc, scratch, nbytes, B, H, W, V, flags, stream):
        nc = 126 if V == 5 else 35
        self.seen["layer"] = (V, self._table(c, B * 3 * nc).reshape(B, 3, nc))
        np.ctypeslib.as_array(ctypes.cast(gc, ctypes.POINTER(ctypes.c_float)), (B * 3 * nc,))[:] = np.arange(B * 3 * nc)
        return 0


@pytest.mark.parametrize("d,V,n", R.NEW_COUNTS, ids=R.COUNT_IDS)
def test_backward_pads_to_order_4_and_cuts_the_gradient_back(monkeypatch, d, V, n):
    """ops.trispace_backward / trispace_backward_img / poly_layer_backward on an order-d table hand the library the order-4
    table of the same polynomials -- the table's n entries, then zeros -- and return gradients of the table's own width: the
    first n entries of every order-4 row."""
    from curl_amd import _lib, ops
    rec = _Recorder()
    monkeypatch.setattr(ops, "_need_device", lambda t, name: None)
    monkeypatch.setattr(ops, "_stream", lambda t: None)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    n4 = R.n_coeffs(4, V)
    g = torch.Generator().manual_seed(n)
    img, w = torch.rand(2, 3, 4, 4, generator=g), torch.rand(2, 3, 4, 4, generator=g)
    c = torch.randn(2, 3, 3, n, generator=g)
    got = ops.trispace_backward(img, c, w)
    nc, table, mis = rec.seen["bwd"]
    assert nc == n4 and mis == 0 and np.array_equal(table[..., :n], c.numpy()) and not table[..., n:].any()
    assert got.shape == (2, 3, 3, n) and got.is_contiguous()
    assert np.array_equal(got.numpy(), np.arange(2 * 9 * n4, dtype=np.float32).reshape(2, 3, 3, n4)[..., :n])
    assert ops.trispace_backward_img(img, c, w).shape == img.shape
    nc, table, mis = rec.seen["bwd_img"]
    assert nc == n4 and mis == 0 and np.array_equal(table[..., :n], c.numpy()) and not table[..., n:].any()
    x = torch.rand(2, V, 4, 4, generator=g)
    gi, gc = ops.poly_layer_backward(x, c[:, 0], w)
    Vs, table = rec.seen["layer"]
    assert Vs == V and np.array_equal(table[..., :n], c[:, 0].numpy()) and not table[..., n:].any()
    assert gi.shape == x.shape and gc.shape == (2, 3, n)
    assert np.array_equal(gc.numpy(), np.arange(2 * 3 * n4, dtype=np.float32).reshape(2, 3, n4)[..., :n])


def test_malformed_tables_name_the_lower_order_widths(monkeypatch):
    from curl_amd import ops
    monkeypatch.setattr(ops, "_need_device", lambda t, name: None)
    img = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match=r"coeffs must be \[B=2,3,3,126\|35\], got \(2, 3, 3, 57\).*56\|20, 21\|10, 6\|4"):
        ops.trispace_forward(img, torch.zeros(2, 3, 3, 57))
    with pytest.raises(ValueError, match=r"coeffs must be \[B=2,3,35\], got \(2, 3, 21\).*20, 10, 4"):
        ops.poly_layer(img, torch.zeros(2, 3, 21))  # 21 is a 5-variable width


# ------------------------------------------------------------------ the generated schemes and their host twin
@pytest.fixture(scope="module", params=FLAVOURS)
def orders_twin(request):
    """The two flavours of conftest's `twin` fixture, for this twin's own source file."""
    return twin_library("poly_orders_twin.cpp", request.param)


def _P(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _twin_layer(lib, x, c, d, seq):
    x, c = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(c, np.float32)
    B, V, H, W = x.shape
    assert c.shape == (B, 3, R.n_coeffs(d, V))
    out = np.empty((B, 3, H, W), np.float32)
    assert lib.twin_poly_order_layer(_P(x), _P(c), _P(out), B, ctypes.c_long(H * W), V, d, int(seq)) == 0
    return out


@pytest.mark.parametrize("V", [5, 3])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_twin_orders_against_float64_and_against_order_4(orders_twin, golden, d, V):
    """The order-d Horner scheme on the inputs of poly.npz with coefficient prefixes: against O.channel_poly_layer in float64,
    and against the twin's own order-4 scheme on the zero-padded table.  Bound: the 3e-6 tests/test_poly.py holds degree 4 to
    -- a shorter chain of the same operations rounds no more often."""
    g = golden("poly")
    x, c4 = g[f"x{V}"], g[f"c{V}"]
    n = R.n_coeffs(d, V)
    c = np.ascontiguousarray(c4[..., :n])
    want = O.channel_poly_layer(t(x).double(), t(c).double(), d).numpy()
    padded = np.zeros_like(c4)
    padded[..., :n] = c
    via4 = _twin_layer(orders_twin, x, padded, 4, True)
    for seq in (False, True):
        got = _twin_layer(orders_twin, x, c, d, seq)
        assert max_err(got, want) <= 3e-6, (d, V, seq)
        assert max_err(got, via4) <= 3e-6, (d, V, seq)
    if d < 4:
        ref = golden("poly_orders")[f"channel_poly_d{d}v{V}"]
        assert max_err(_twin_layer(orders_twin, x, c, d, True), ref) <= 3e-6


@pytest.mark.parametrize("V", [5, 3])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_consumption_order_tables(orders_twin, d, V):
    """kPolyOrder_d{d}_v{V} is a permutation of range(n(d, V)) -- every coefficient is consumed once -- and names monomials of
    generate_powers(d, V): the graded order makes index q < n(d, V) the same monomial at order d as at order 4.  The staged
    stride is a multiple of 4 floats that holds the table."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_poly_horner as gph
    from curl_amd.model import ChannelPolyLayer
    n = R.n_coeffs(d, V)
    buf = (ctypes.c_int * 128)()
    assert orders_twin.twin_poly_order_table(V, d, buf) == n
    table = list(buf[:n])
    assert sorted(table) == list(range(n))
    mine = [tuple(p) for p in ChannelPolyLayer.generate_powers(d, V)]
    assert mine == gph.powers(d, V) == gph.powers(4, V)[:n]
    # the scheme is Horner in variable 0 first: the first coefficient consumed is the top power of variable 0 ...
    assert mine[table[0]] == (d,) + (0,) * (V - 1)
    # ... and its text in the generated file is the generator's own, table included
    text = open(os.path.join(ROOT, "curl_amd", "csrc", "poly_horner.inc")).read()
    assert f"kPolyOrder_d{d}_v{V}[{n}] = {{{', '.join(map(str, table))}}};" in text
    assert gph.gen(d, V)[1] in text
    stride = orders_twin.twin_poly_order_stride(V, d)
    assert stride % 4 == 0 and n <= stride < n + 4


# ------------------------------------------------------------------ the composed oracle against the reference's outputs
@pytest.mark.parametrize("d", [1, 2, 3])
def test_oracle_layers_match_the_reference(golden, d):
    g, go = golden("poly"), golden("poly_orders")
    for V in (5, 3):
        n = R.n_coeffs(d, V)
        got = O.channel_poly_layer(t(g[f"x{V}"]), t(g[f"c{V}"][..., :n]), d).numpy()
        assert np.allclose(got, go[f"channel_poly_d{d}v{V}"], rtol=0, atol=2e-6)


@pytest.mark.parametrize("s", ["s02", "s1"])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_composed_oracle_matches_the_reference(golden, d, s):
    """tests/poly_orders_ref.py's trispace_residual against TriSpaceRegNet.generate_residual / generate_image of the reference
    with ChannelPolyLayer(d): the bound tests/test_poly.py holds the degree-4 oracle to."""
    g, go = golden("poly"), golden("poly_orders")
    c = t(g[s + "_coeffs"][..., :R.n_coeffs(d, 5)])
    for nm in (("img", "img8") if s == "s02" else ("img",)):
        r = R.trispace_residual(t(g[nm]), c[:, 0], c[:, 1], c[:, 2], d)
        assert max_err(r.numpy(), go[f"{s}_{nm}_residual_d{d}v5"]) <= 3e-6
        assert max_err(O.generate_image(t(g[nm]), r).numpy(), go[f"{s}_{nm}_image_d{d}v5"]) <= 3e-6
    c3 = t(g[s + "_coeffs35"][..., :R.n_coeffs(d, 3)])
    r = R.trispace_residual(t(g["img"]), c3[:, 0], c3[:, 1], c3[:, 2], d, spatial=False)
    assert max_err(r.numpy(), go[f"{s}_img_residual_d{d}v3"]) <= 3e-6
    if s == "s02":
        assert max_err(O.generate_image(t(g["img"]), r).numpy(), go[f"{s}_img_image_d{d}v3"]) <= 3e-6


def test_composed_oracle_is_the_oracle_at_degree_4(golden):
    """At degree 4 the helper is oracle.trispace_residual with the ChannelPolyLayer form, bit for bit; and an order-d table is
    its zero-padded order-4 table (float64, to rounding)."""
    g = golden("poly")
    c = t(g["s02_coeffs"])
    a = R.trispace_residual(t(g["img"]), c[:, 0], c[:, 1], c[:, 2], 4)
    assert torch.equal(a, O.trispace_residual(t(g["img"]), c[:, 0], c[:, 1], c[:, 2], mobile=False))
    for d, V, n in R.NEW_COUNTS:
        cd = t(g["s02_coeffs" if V == 5 else "s02_coeffs35"][..., :n]).double()
        low = R.trispace(t(g["img"]).double(), cd, residual_only=True)
        full = R.trispace(t(g["img"]).double(), R.pad4(cd), residual_only=True)
        assert float((low - full).abs().max()) <= 1e-12
