"""Operand layouts for the strided-operand parity tests (a plain module, not collected; tests/test_layouts.py is its CPU
self-test).  A layout turns a logical tensor -- (b, s, h, d), ragged (total, h, d) or a page pool (pages, page, hk, d): anything
that ends in (heads, head dim) -- into a view with the same values inside a larger 1-D allocation:

    "padded"        big[..., :h, :d] of a (..., h + 1, d + pad) buffer: one spare head, `pad` spare columns per head
    "padded_wide"   the same with two spare heads and 2 x pad columns (a second stride triple for a same-shaped operand)
    "bhsd"          storage in (b, h, s, d) order seen as (b, s, h, d): row stride d, head stride s x d; ragged (h, total, d);
                    pools (pages, hk, page, d)
    "bhsd_padded"   bhsd storage whose rows carry `pad` spare columns: row stride d + pad, head stride s x (d + pad)
    "misaligned"    "padded" with 4 spare columns: head and row strides are no multiple of 8     | only for the tests of the
    "misaligned_base"  contiguous strides, the view starts 4 elements behind a 16-byte boundary  | binding's copy path
pad = 8 elements for 2- and 4-byte types and 16 for 1-byte ones (fp8 K / V: strides in bytes), so that every stride of the
first four stays a multiple of 8 elements / 16 bytes and the base 16-byte aligned: aligned() / cache_aligned() below are the
binding's own rules (csrc/torch_binding.cpp), which accept these views without a copy.

Every non-contiguous view lies in the interior of its allocation.  In front of it are at least N elements, N = the size of the
contiguous tensor; behind it at least max(N, slack) -- `slack` is given by the caller, call_slack() of the call's operands.
Gaps and slack hold NaN for inputs (NAN_BITS: a NaN of bf16, fp16, e4m3fn and fp32 alike) and the byte 0xA5 for outputs.
What that buys:
  * gap data that reaches a result poisons it (NaN), a store outside the view damages a sentinel;
  * a kernel that applies a wrong stride to the right pointer damages sentinels inside the allocation and does not leave it.
    The strides of this module are never negative, so such an access lies behind the start of the view.  With extents
    B, S, H, D = the largest batch / row / head / column counts of any operand of the call, P = the widest pad and
    X = S (H + 2) (D + 2P), every stride any layout above gives any operand of the call is at most: batch X, row
    (H + 2)(D + 2P) = X / S, head S (D + 2P) = X / (H + 2) (the contiguous strides S H D, H D, D are below them).  An index
    (b, s, h, c) inside the extents, under any mix of those strides, lands at most (B - 1) X + (S - 1) X / S + (H - 1) X / (H + 2)
    + D < (B + 1) X = call_slack elements behind the start of the view: inside the slack.  Wrong pointers, extents read
    from another operand's *shape* beyond B / S / H / D, or a byte / element mix-up by more than the slack are not covered.
    P is the widest pad of the call: over an fp8 cache the strides of K / V count bytes (pad 16) and those of q / o / qv
    elements (pad 8), so that call passes itemsize 1 to call_slack for every allocation, the 16-bit ones included.

mixed assignments (ASSIGNMENTS): which layout each operand of a call gets.  No two operands of one call that can have the same
shape -- q / o / qv, q / o / do / dq, k / v / dk / dv -- share a layout, so none share a stride triple; across the two
assignments every operand gets a padded and a bhsd layout.  Page pools are always padded views ("k_pages" / "v_pages")."""
import math

import torch

INT = {1: torch.int8, 2: torch.int16, 4: torch.int32}
NAN_BITS = {1: 0x7F, 2: 0x7FFF, 4: 0x7FFFFFFF}                   # inputs: a NaN in every element type the kernels read
SENTINEL_BITS = {1: -0x5B, 2: -0x5A5B, 4: -0x5A5A5A5B}           # outputs: the byte 0xA5 (as signed integers)

# name -> (storage order, spare heads, spare columns in units of pad (negative: in elements), elements the base is moved by)
LAYOUTS = {
    "contiguous": ("bshd", 0, 0, 0),
    "padded": ("bshd", 1, 1, 0),
    "padded_wide": ("bshd", 2, 2, 0),
    "bhsd": ("bhsd", 0, 0, 0),
    "bhsd_padded": ("bhsd", 0, 1, 0),
    "misaligned": ("bshd", 1, -4, 0),
    "misaligned_base": ("bshd", 0, 0, 4),
}
ALIGNED_LAYOUTS = ("padded", "padded_wide", "bhsd", "bhsd_padded")
MISALIGNED_LAYOUTS = ("misaligned", "misaligned_base")

ASSIGNMENTS = (
    dict(q="padded", k="bhsd", v="padded", o="bhsd", qv="padded_wide", do="padded_wide", dq="bhsd_padded", dk="padded_wide",
         dv="bhsd_padded", k_pages="padded", v_pages="padded_wide"),
    dict(q="bhsd", k="padded", v="bhsd", o="padded", qv="bhsd_padded", do="bhsd_padded", dq="padded_wide", dk="bhsd_padded",
         dv="padded_wide", k_pages="padded_wide", v_pages="padded"),
)
SAME_SHAPE_GROUPS = (("q", "o", "qv"), ("q", "o", "do", "dq"), ("k", "v", "dk", "dv"), ("k_pages", "v_pages"))


def pad_of(itemsize):
    return 16 if itemsize == 1 else 8


def aligned(t):
    """csrc/torch_binding.cpp aligned(): what the dense / varlen / backward entry points take without a copy."""
    return t.data_ptr() % (16 if t.element_size() == 2 else 8) == 0 and all(s % 8 == 0 for s in t.stride()[:-1])


def cache_aligned(t, base_grain=16, stride_grain=8):
    """csrc/torch_binding.cpp cache_aligned(): what a KV cache must satisfy (an fp8 cache: grains 16 / 16); it is never copied."""
    return t.data_ptr() % base_grain == 0 and all(s % stride_grain == 0 for s in t.stride()[:3])


def call_slack(shapes, itemsize=2):
    """Elements behind every view of a call whose operands have `shapes`: see the module docstring."""
    lead = [math.prod(s[:-3]) if len(s) > 3 else 1 for s in shapes]
    B, S = max(lead), max(s[-3] for s in shapes)
    H, D = max(s[-2] for s in shapes), max(s[-1] for s in shapes)
    return (B + 1) * S * (H + 2) * (D + 2 * pad_of(itemsize))


def geometry(shape, itemsize, layout, slack=0):
    """-> (elements of the allocation, offset of the view, strides of the view)."""
    order, heads, cols, shift = LAYOUTS[layout]
    *lead, h, d = shape
    n = math.prod(shape)
    if layout == "contiguous":
        return n, 0, tuple(torch.empty(shape, device="meta").stride())
    dp = d + (cols * pad_of(itemsize) if cols >= 0 else -cols)
    if order == "bshd":
        store = (*lead, h + heads, dp)
        strides = torch.empty(store, device="meta").stride()
    else:
        store = (*lead[:-1], h, lead[-1], dp)
        st = torch.empty(store, device="meta").stride()
        strides = (*st[:-3], st[-2], st[-3], st[-1])
    up = lambda x: -(-x // 16) * 16  # noqa: E731  (the view starts on a 16-element boundary: 16 bytes for fp8, more otherwise)
    before, after = up(n), up(max(n, slack))
    return before + math.prod(store) + after + shift, before + shift, tuple(strides)


class Placed:
    """A logical tensor inside its allocation.  `view` has the logical shape; `buf` is the whole 1-D allocation."""

    def __init__(self, shape, dtype, layout, device, fill_bits, slack=0):
        self.layout, self.shape, self.itemsize = layout, tuple(shape), torch.empty((), dtype=dtype).element_size()
        numel, self.offset, self.strides = geometry(self.shape, self.itemsize, layout, slack)
        self.fill = fill_bits[self.itemsize]
        self.bits = torch.full((numel,), self.fill, dtype=INT[self.itemsize], device=device)
        self.buf = self.bits.view(dtype)
        self.view = self.buf.as_strided(self.shape, self.strides, self.offset)

    def view_bits(self, of=None):
        return (self.bits if of is None else of).as_strided(self.shape, self.strides, self.offset)

    def intact(self):
        """Every element of the allocation outside the view still holds the fill pattern."""
        probe = self.bits.clone()
        self.view_bits(probe).fill_(self.fill)
        return bool((probe == self.fill).all())

    def holds(self, x):
        """The view holds the bits of x (NaN-safe, sign-of-zero-safe)."""
        return torch.equal(self.view_bits(), x.to(self.bits.device).contiguous().view(INT[self.itemsize]))


def place_input(x, layout, device="cpu", slack=0):
    """The values of x as a `layout` view on `device`, NaN around and between them."""
    p = Placed(x.shape, x.dtype, layout, device, NAN_BITS, slack)
    p.view_bits().copy_(x.contiguous().view(INT[p.itemsize]).to(device))
    return p


def place_output(shape, dtype, layout, device="cpu", slack=0):
    """An output view of `shape`: the whole allocation, the view included, holds the sentinel byte."""
    return Placed(shape, dtype, layout, device, SENTINEL_BITS, slack)
