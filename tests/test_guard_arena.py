"""The guard-band arena (tests/guard_arena.py) held to planted defects, on the CPU: stand-in "entry points" written in torch
each break one rule, and the matching check must fire and name the buffer and the side.  Then the layout's properties over
many sizes, and that the GPU sweep's table (tests/test_gpu_guard_bands.py) has a row for every pointer-taking entry point."""
import itertools

import pytest
import torch

import guard_arena as GA
from guard_arena import GUARD, IN, INOUT, OUT, WORK, Buf, GuardError, Layout, run_both

N = 37  # floats: no multiple of 4


def bufs(n=N):
    x = torch.arange(n, dtype=torch.float32) * 0.25 + 1.0
    return [Buf("x", IN, x), Buf("y", OUT, shape=(n,), dtype=torch.float32), Buf("scratch", WORK, nbytes=48, grid=16)]


def f32_at(A, byte_offset, n):
    return A.bytes[byte_offset:byte_offset + 4 * n].clone().view(torch.float32)


def doubling(A):
    """y = 2 x; the scratch is scribbled on (its contents are nobody's business)"""
    A.write("y", 2.0 * A.read("x"))
    A.write("scratch", torch.full((12,), 7.0))


@pytest.mark.parametrize("cls", GA.CLASSES)
def test_a_correct_call_passes_and_its_outputs_can_be_read(cls):
    A = run_both(bufs(), cls, "cpu", doubling)
    assert torch.equal(A.read("y"), 2.0 * bufs()[0].data)
    assert A.ptr("y") % 16 == (0 if cls == "16" else 4) and A.ptr("scratch") % 16 == 0 and A.ptr("absent") == 0
    assert A.nbytes("scratch") == 48 and A.nbytes("absent") == 0


def expect(check, buffer, side, offset, call, cls="16+4", b=None):
    with pytest.raises(GuardError) as e:
        run_both(b or bufs(), cls, "cpu", call)
    err = e.value
    assert (err.check, err.buffer, err.side, err.offset) == (check, buffer, side, offset), str(err)


@pytest.mark.parametrize("cls", GA.CLASSES)
def test_one_byte_before_a_buffer(cls):
    def call(A):
        doubling(A)
        A.bytes[A.off("y") - 1] = 0
    expect("guard", "y", "before", -1, call, cls)


@pytest.mark.parametrize("cls", GA.CLASSES)
def test_one_element_after_a_buffer(cls):
    def call(A):
        doubling(A)
        end = A.off("y") + 4 * N
        A.bytes[end:end + 4] = torch.tensor([2.0]).view(torch.uint8)
    expect("guard", "y", "after", 0, call, cls)


def test_a_store_far_into_the_band_after_the_scratch():
    def call(A):
        doubling(A)
        A.bytes[A.off("scratch") + 48 + GUARD - 1] = 0
    expect("guard", "scratch", "after", GUARD - 1, call)


def test_the_last_element_of_an_output_left_unwritten():
    def call(A):
        A.write("y", (2.0 * A.read("x"))[:-1])
    expect("unwritten", "y", "buffer", 4 * (N - 1), call)


def test_an_unwritten_byte_output_is_caught_too():
    b = [Buf("x", IN, torch.arange(40, dtype=torch.uint8)), Buf("y", OUT, shape=(40,), dtype=torch.uint8)]

    def call(A):
        A.write("y", A.read("x")[:36])
    expect("unwritten", "y", "buffer", 36, call, b=b)


def test_a_result_that_depends_on_the_element_after_an_input():
    def call(A):
        x = f32_at(A, A.off("x"), N + 1)  # one float too many
        A.write("y", 2.0 * x[:N] + 0.001 * torch.nan_to_num(x[1:], nan=3.0))  # the last term: poison, read as a number
    expect("poison", "y", "buffer", 4 * (N - 1), call)


def test_an_input_modified():
    def call(A):
        doubling(A)
        A.bytes[A.off("x") + 9] ^= 0x40
    expect("input", "x", "buffer", 9, call)


def slab_bufs(H=6, W=5, r0=2, n=3):
    x = torch.rand(H, W, generator=torch.Generator().manual_seed(1))
    return [Buf("x", IN, x), Buf("y", OUT, shape=(H, W), dtype=torch.float32, keep=[(0, r0 * W * 4), ((r0 + n) * W * 4, H * W * 4)])]


def slab_call(rows):
    def call(A):
        x, W = A.read("x"), 5
        for r in rows:
            o = A.off("y") + r * W * 4
            A.bytes[o:o + W * 4] = (2.0 * x[r]).contiguous().view(torch.uint8)
    return call


def test_a_slab_call_keeps_the_rows_outside_it():
    A = run_both(slab_bufs(), "16", "cpu", slab_call((2, 3, 4)))
    assert torch.equal(A.read("y")[2:5], 2.0 * slab_bufs()[0].data[2:5])


def test_a_row_written_outside_its_slab():
    expect("inner", "y", "inner", 5 * 5 * 4, slab_call((2, 3, 4, 5)), b=slab_bufs())
    expect("inner", "y", "inner", 1 * 5 * 4, slab_call((1, 2, 3, 4)), b=slab_bufs())
    expect("unwritten", "y", "buffer", 4 * 5 * 4, slab_call((2, 3)), b=slab_bufs())


def test_an_in_place_value_is_compared_between_the_runs_but_never_called_unwritten():
    def b():
        return [Buf("reg", INOUT, torch.tensor([0.5, 1.5])), Buf("y", OUT, shape=(2,), dtype=torch.float32)]

    def ok(A):
        A.write("reg", A.read("reg") + 1.0)
        A.write("y", torch.ones(2))
    assert torch.equal(run_both(b(), "16+4", "cpu", ok).read("reg"), torch.tensor([1.5, 2.5]))
    run_both(b(), "16", "cpu", lambda A: A.write("y", torch.ones(2)))  # left alone: not an assignment anyone owes

    def leaky(A):
        A.write("reg", A.read("reg") + f32_at(A, A.off("reg") + 8, 2))
        A.write("y", torch.ones(2))
    expect("poison", "reg", "buffer", 0, leaky, b=b())


def test_the_poison_words():
    a, b = (torch.tensor([w - (1 << 32) if w >> 31 else w], dtype=torch.int32) for w in (GA.POISON_A, GA.POISON_B))
    assert torch.isnan(a.view(torch.float32)).all() and torch.isfinite(b.view(torch.float32)).all()
    ab, bb = a.view(torch.uint8), b.view(torch.uint8)
    assert (ab != 0).all() and (bb != 0).all() and (ab != bb).all()
    assert GUARD == 256 * 1024


SIZES = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 33, 255, 256, 257, 4095, 4097, 65536 + 12, GUARD, GUARD + 4]


@pytest.mark.parametrize("cls", GA.CLASSES)
def test_layout_properties(cls):
    kinds = [(torch.float32, None), (torch.uint8, None), (torch.float64, None), (torch.float32, 16), (torch.float32, 8), (torch.uint8, 16)]
    for (n0, n1, n2), shift in zip(itertools.product(SIZES[::3], SIZES[1::3], SIZES[2::3]), itertools.cycle(range(len(kinds)))):
        spec = []
        for i, n in enumerate((n0, n1, n2)):
            dtype, grid = kinds[(i + shift) % len(kinds)]
            size = torch.empty(0, dtype=dtype).element_size()
            spec.append(Buf(f"b{i}", WORK if grid else OUT, nbytes=n * size, dtype=dtype, grid=grid))
        L = Layout(spec, cls)
        regions = L.regions()
        assert regions[0][0] == 0 and regions[-1][1] == L.total
        for (lo, hi, _, _), (lo2, _, _, _) in zip(regions, regions[1:]):
            assert lo < hi and hi == lo2  # address order, no overlap, no gap nobody checks
        for b in spec:
            off = L.off[b.name]
            if cls == "16" or b.grid == 16:
                assert off % 16 == 0
            elif b.grid == 8:
                assert off % 16 == 8
            else:
                assert off % 16 == {1: 1, 4: 4, 8: 8}[b.itemsize]
            assert off % b.itemsize == 0
            assert L.before[b.name][1] == off and off - L.before[b.name][0] >= GUARD   # the band ends at the buffer's first byte
            assert L.after[b.name] == (off + b.nbytes, off + b.nbytes + GUARD)         # ... and starts again at the very next one


def test_the_sweep_has_a_row_for_every_pointer_taking_entry_point():
    import test_gpu_guard_bands as T
    want = T.pointer_taking_entries()
    assert "curl_layer_bwd_f32" in want and "curl_trispace_bwd_img_f32" in want and "curl_workspace_bytes" not in want
    got = T.covered_entries()
    assert got == want, (sorted(want - got), sorted(got - want))
    assert all(r.shapes for r in T.ROWS)
