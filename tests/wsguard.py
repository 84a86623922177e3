"""Guard band behind a kernel workspace.  A test that allocates a workspace
itself hands the library exactly the size the library reported; behind it lie
4 KB of a byte pattern that must survive the call -- so the reported size is
shown, on the real kernels, to cover what they carve."""
BAND = 4096
PATTERN = 0xA5
SHIFT = 0          # default `shift`; a test that wants its base moved patches it


class Guarded:
    """`nbytes` of workspace on `device`, the band behind it.  `shift` moves
    the base that many bytes off the allocation's own (256-aligned) start, so
    that the library has to spend its alignment slack."""

    def __init__(self, nbytes, device="cuda", shift=None):
        import torch
        shift = SHIFT if shift is None else shift
        self.nbytes, self.shift = int(nbytes), shift
        # (the pattern all over: a workspace may hold anything)
        self.buf = torch.full((shift + self.nbytes + BAND,), PATTERN, dtype=torch.uint8,
                              device=device)
        assert self.buf.data_ptr() % 256 == 0
        self.tensor = self.buf[shift:shift + self.nbytes]     # what the library gets

    def data_ptr(self):
        return self.tensor.data_ptr()

    def check(self):
        """Synchronises; the bytes around the workspace are untouched."""
        import torch
        torch.cuda.synchronize(self.buf.device)
        end = self.shift + self.nbytes
        assert bool((self.buf[end:] == PATTERN).all()), "write behind the workspace"
        assert bool((self.buf[:self.shift] == PATTERN).all()), "write ahead of the workspace"
