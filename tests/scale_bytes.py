"""Plain helpers of tests/test_gpu_scale_bytes.py: byte content made on the device, the ragged arenas' layout as index
tensors, and the pre-filled out arena.  Nothing here computes an expected value with the library's kernels."""
import contextlib

import torch

POISON = 0xA5  # what the out arena holds before a ragged entry runs
MASK_LEVELS = (0, 1, 128, 255)


def rand_u8(g, dev, *shape):
    """Random bytes made on the device (no int64 temporaries: uint8.random_)."""
    return torch.empty(shape, dtype=torch.uint8, device=dev).random_(0, 256, generator=g)


def level_bytes(g, dev, *shape):
    """Bytes drawn from {0, 1, 128, 255}, made on the device 64 M at a time."""
    lut = torch.tensor(MASK_LEVELS, dtype=torch.uint8, device=dev)
    out = torch.empty(shape, dtype=torch.uint8, device=dev)
    flat = out.view(-1)
    for a in range(0, flat.numel(), 1 << 26):
        part = flat[a:a + (1 << 26)]
        part.copy_(lut[torch.empty(part.numel(), dtype=torch.uint8, device=dev).random_(0, 4, generator=g).long()])
    return out


def banded_mask(g, dev, *shape):
    """A uint8 mask [..., H, W]: of every eight rows two are 0 from end to end (whole wavefronts skip in the foreground entries),
    two are 255 and four are drawn from {0, 1, 128, 255}."""
    m = level_bytes(g, dev, *shape)
    for r, v in ((0, 0), (5, 0), (2, 255), (3, 255)):
        m[..., r::8, :] = v
    return m


def fill_periodic(image, tile):
    """image [H,W,C] (a view into an arena) <- tile [8,W,C] repeated down the rows."""
    H = image.shape[0]
    full = H // 8
    image[:full * 8].view(full, -1).copy_(tile.reshape(1, -1).expand(full, -1))
    image[full * 8:].copy_(tile[:H - full * 8])


def differs_from_periodic(image, block=512):
    """The number of elements of image [H,W,...] that differ from the image's first eight rows repeated, counted on the device
    `block` row blocks at a time."""
    H = image.shape[0]
    full = H // 8
    first = image[:8].reshape(1, -1)
    rows = image[:full * 8].view(full, -1)
    bad = 0
    for a in range(0, full, block):
        bad += int((rows[a:a + block] != first).sum())
    return bad + int((image[full * 8:] != image[:H - full * 8]).sum())


def int_sse(a, b, mask=None, rows=1024):
    """(sum over the pixels whose mask byte is not 0 and the channels of (a - b)^2, the number of those pixels) of two byte
    images [H,W,3] on the device: torch integer arithmetic, `rows` rows at a time, int64 sums.  Python ints."""
    sse = n = 0
    for r in range(0, a.shape[0], rows):
        d = a[r:r + rows].to(torch.int32) - b[r:r + rows].to(torch.int32)
        sq = (d * d).sum(dim=2)
        if mask is None:
            n += sq.numel()
        else:
            keep = mask[r:r + rows] != 0
            sq = sq * keep
            n += int(keep.sum())
        sse += int(sq.sum(dtype=torch.int64))
    return sse, n


def score_tiles(h, w):
    """(class, workgroups) of an H x W image in the flat tiling of 256 lanes: four pixels per lane where H*W % 4 == 0 (the dword
    class), one otherwise (the byte class) -- include/curl_hip_ragged.h."""
    px = h * w
    return ("dword", -(-(px // 4) // 256)) if px % 4 == 0 else ("byte", -(-px // 256))


def plan_tiles(ops, shapes):
    """The tile count of every image from the library's host plan of operator 0 (descriptor word 8, image order)."""
    plan = ops._ragged_plan([tuple(s) for s in shapes], [3] * len(shapes), False, 0, None)
    d = plan.host.numpy()[32:32 + 16 * len(shapes)].reshape(len(shapes), 16)
    tiles = [0] * len(shapes)
    for row in d:
        tiles[int(row[1])] = int(row[8])
    return tiles


class Layout:
    """The three arenas of a shape list [(H, W, C)] as the library lays them out, and index tensors into them per shape group."""

    def __init__(self, ops, shapes, dev):
        self.ops, self.dev = ops, dev
        self.shapes = [(int(h), int(w)) for h, w, _ in shapes]
        self.channels = [int(c) for _, _, c in shapes]
        B = len(shapes)
        self.img_off, self.img_bytes = ops.RaggedBytes.layout(self.shapes, self.channels)
        self.mask_off, self.mask_bytes = ops.RaggedBytes.layout(self.shapes, [1] * B)
        self.out_off, self.out_bytes = ops.RaggedBytes.layout(self.shapes, [3] * B)
        self.groups = {}  # (H, W, C) -> the indices of its images, ascending
        for i, s in enumerate(shapes):
            self.groups.setdefault(tuple(int(v) for v in s), []).append(i)

    def ragged(self, arena, kind):
        """A RaggedBytes over `arena`: kind 'img' | 'mask' | 'out'."""
        off, ch = {"img": (self.img_off, self.channels), "mask": (self.mask_off, [1] * len(self.shapes)),
                   "out": (self.out_off, [3] * len(self.shapes))}[kind]
        return self.ops.RaggedBytes(arena, self.shapes, off, ch)

    def index(self, key, kind):
        """int64 [n, H*W*c] on the device: the arena positions of the bytes of every image of shape group `key`."""
        h, w, c = key
        off, c = {"img": (self.img_off, c), "mask": (self.mask_off, 1), "out": (self.out_off, 3)}[kind]
        first = torch.tensor([off[i] for i in self.groups[key]], dtype=torch.int64, device=self.dev)
        return first[:, None] + torch.arange(h * w * c, dtype=torch.int64, device=self.dev)[None, :]

    def ids(self, key):
        return torch.tensor(self.groups[key], dtype=torch.int64, device=self.dev)

    def padding(self, kind="out"):
        """int64 [k] on the device: every arena position that belongs to no image (the gaps in front of the 16-byte offsets)."""
        off, ch, total = {"img": (self.img_off, self.channels, self.img_bytes), "mask": (self.mask_off, [1] * len(self.shapes), self.mask_bytes),
                          "out": (self.out_off, [3] * len(self.shapes), self.out_bytes)}[kind]
        start = torch.tensor(off, dtype=torch.int64)
        size = torch.tensor([h * w * c for (h, w), c in zip(self.shapes, ch)], dtype=torch.int64)
        end = start + size
        gap = torch.cat([start[1:], torch.tensor([total], dtype=torch.int64)]) - end
        assert int(start[0]) == 0 and int(gap.min()) >= 0 and int(gap.max()) < 16  # the layout leaves alignment padding only
        pos = end[:, None] + torch.arange(16, dtype=torch.int64)[None, :]
        return pos[torch.arange(16)[None, :] < gap[:, None]].to(self.dev)


@contextlib.contextmanager
def prefilled_out(ops):
    """Inside the block every ragged forward entry finds its out arena filled with POISON (ops allocates it uninitialised):
    the fill is enqueued on the entry's stream in front of its launches."""
    plain = ops._ragged_arenas

    def filled(rb, wm, nc_arg):
        plan, out = plain(rb, wm, nc_arg)
        out.arena.fill_(POISON)
        return plan, out
    ops._ragged_arenas = filled
    try:
        yield
    finally:
        ops._ragged_arenas = plain
