"""Guard bands for kernel tests: every region a kernel reads or writes lives inside a larger tensor of
the same allocation.  Read regions are surrounded by NaN (an over-read poisons a sum), written regions
by a sentinel; after the launch the surroundings must be bit-unchanged.  This finds out-of-range
addressing without any access outside an allocation."""
import torch

PAD = 64   # elements on each side (>= 64 bytes for every dtype: the region keeps its 16-byte alignment)
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bit patterns as integers (NaN-safe equality)."""
    return t.view(_BITS[t.element_size()])


class Band:
    def __init__(self, n: int, dtype, guard, dev="cuda"):
        self.n = int(n)
        self.full = torch.full((self.n + 2 * PAD,), guard, dtype=dtype, device=dev)
        self.v = self.full[PAD:PAD + self.n]
        self._guard = bits(self.full).clone()

    def set(self, src) -> "Band":
        if isinstance(src, torch.Tensor):
            self.v.copy_(src.reshape(-1).to(self.v.dtype))
        else:
            self.v.fill_(src)
        return self

    def ptr(self) -> int:
        return self.v.data_ptr()

    def guards_intact(self) -> bool:
        b = bits(self.full)
        e = PAD + self.n
        return torch.equal(b[:PAD], self._guard[:PAD]) and torch.equal(b[e:], self._guard[e:])

    def snap(self) -> torch.Tensor:
        return bits(self.full).clone()

    def same(self, snap: torch.Tensor) -> bool:
        return torch.equal(bits(self.full), snap)

    def cpu(self) -> torch.Tensor:
        return self.v.detach().cpu().clone()
