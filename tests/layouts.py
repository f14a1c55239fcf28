"""Operand layouts for the C-ABI tests (include/lasso_hip.h: "row-major with an explicit leading dimension in elements").
TEST INFRASTRUCTURE, plain torch: a matrix is placed as a view of a larger buffer so that the leading dimension and the
base pointer's alignment are the ones a host with its own allocator hands in, and whatever lies between the rows is poison.

  natural   ld = row length, the buffer's own (allocator-aligned) base
  pitched   ld = row length rounded up to a multiple of 4 (8 for bf16) plus 8; base 16-byte aligned: the vector forms run
            with ld != row length
  odd       ld = row length + 3 (+ 5 where that is a multiple of 4): ld % 4 != 0, the scalar forms run on shapes whose
            row length alone would allow vectors
  offset    ld a multiple of 4, the base moved by ONE element: aligned to the element only -- only a guard that looks at
            the pointer says no

Inputs carry NaN in the padding (and in the element in front of an `offset` base): a result that contains NaN depends on
memory that is not part of the operand.  Outputs are a whole buffer of a sentinel.  check() afterwards: the padding is
bit for bit what it was, and -- inputs -- so is the operand."""
import torch

LAYOUTS = ("natural", "pitched", "odd", "offset")
SENTINEL = -7.25
_BITS = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16, torch.float16: torch.int16,
         torch.int32: torch.int32}


def leading_dimension(cols, layout, dtype=torch.float32):
    """(ld, elements in front of the base) of a [rows][cols] operand in `layout`"""
    vec = 8 if dtype in (torch.bfloat16, torch.float16) else 4
    if layout == "natural":
        return cols, 0
    if layout == "pitched":
        return (cols + vec - 1) // vec * vec + 8, 0
    if layout == "odd":
        ld = cols + 3
        return (ld if ld % 4 else cols + 5), 0
    if layout == "offset":
        return (cols + vec - 1) // vec * vec + vec, 1
    raise ValueError("layout %r" % (layout,))


class Placed:
    """view: the [rows][cols] operand (stride (ld, 1)) inside `buffer`; ld, layout; check(written) -> None or raises"""

    def __init__(self, view, buffer, front, ld, layout, name):
        self.view, self.buffer, self.front, self.ld, self.layout, self.name = view, buffer, front, ld, layout, name
        rows, cols = view.shape
        self._before = buffer.clone()
        inside = torch.zeros(buffer.numel() - front, dtype=torch.bool, device=buffer.device).view(rows, ld)
        inside[:, :cols] = True
        self._inside = torch.cat([torch.zeros(front, dtype=torch.bool, device=buffer.device), inside.reshape(-1)])

    def _bits(self, t):
        return t.view(_BITS[t.dtype])

    def check(self, written=False):
        """the padding (every element of the buffer outside the operand) is bit for bit what place() left there;
        written=False (an input): so is the operand itself"""
        same = self._bits(self.buffer) == self._bits(self._before)
        bad = ~same & ~self._inside
        assert not bool(bad.any()), "%s (%s, ld %d): %d padding elements were written, first at buffer offset %d" % (
            self.name, self.layout, self.ld, int(bad.sum()), int(bad.nonzero()[0]))
        if not written:
            bad = ~same & self._inside
            assert not bool(bad.any()), "%s (%s): an input operand was modified (%d elements)" % (
                self.name, self.layout, int(bad.sum()))

    def reset(self, t_cpu):
        """the operand back to t_cpu (in/out operands between two calls); the padding is left as it is"""
        self.view.copy_(t_cpu.to(self.view.device))
        self._before = self.buffer.clone()


def place(t_cpu, layout, poison, device=None, name="operand", fill=None):
    """A [rows][cols] CPU tensor as a view of a larger buffer on `device` (default: where t_cpu lives) in `layout`.
    poison: what the padding holds (NaN for inputs, SENTINEL for outputs).  fill: None -> the operand holds t_cpu
    (an input); a number -> the operand holds it too (an output: the whole buffer is the sentinel)."""
    assert t_cpu.dim() == 2
    rows, cols = t_cpu.shape
    device = t_cpu.device if device is None else torch.device(device)
    ld, front = leading_dimension(cols, layout, t_cpu.dtype)
    buffer = torch.full((front + rows * ld,), poison, dtype=t_cpu.dtype, device=device)
    view = buffer[front:].view(rows, ld)[:, :cols]
    if fill is None:
        view.copy_(t_cpu.to(device))
    else:
        view.fill_(fill)
    if layout != "offset":
        assert view.data_ptr() % 16 == 0
    else:
        assert view.data_ptr() % 16 == t_cpu.element_size() % 16 and ld % 4 == 0
    assert (rows == 1 or view.stride(0) == ld) and view.stride(1) == 1
    return Placed(view, buffer, front, ld, layout, name)


def plans(names, order=("pitched", "odd", "offset")):
    """The layout matrix of one call: every operand natural (the anchor) -- then one operand at a time in each other
    layout -- then all operands odd, all operands offset.  -> [(tag, {name: layout})], natural and pitched first, offset
    last."""
    out = [("natural", {nm: "natural" for nm in names})]
    for lay in order:
        for nm in names:
            plan = {m: "natural" for m in names}
            plan[nm] = lay
            out.append(("%s-%s" % (nm, lay), plan))
        if lay in ("odd", "offset"):
            out.append(("all-%s" % lay, {nm: lay for nm in names}))
    return out
