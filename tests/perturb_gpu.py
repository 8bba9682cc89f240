"""What the device tests of the two perturbation heads share (tests/test_gpu_faith.py, tests/test_gpu_rise.py): arrays to and
from the device, an output buffer between guard bytes, and frames whose fp32 values are random bit patterns.  Each head's ops,
handles and restatements stay in its own file."""
import numpy as np
import torch

GUARD = 64
PAT = 0xA5


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


class Out:
    """nbytes of device output, `off` bytes into a 16-byte aligned buffer, with GUARD bytes of PAT on either side."""
    def __init__(self, nbytes, off=0):
        self.nbytes, self.lo = nbytes, GUARD + off
        self.t = torch.full((GUARD + 16 + nbytes + GUARD,), PAT, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.lo

    def get(self, dtype, shape):
        host_ = self.t.cpu().numpy()
        assert (host_[:self.lo] == PAT).all() and (host_[self.lo + self.nbytes:] == PAT).all(), "a guard byte was written"
        return host_[self.lo:self.lo + self.nbytes].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.t == PAT).all())


def last_error(lib):
    return lib.fav_last_error(None).decode()


def frames_of(n, H_, W, dtype, seed=0):
    """uint8: random bytes.  float32: random BIT PATTERNS (NaNs of both kinds, infinities and subnormals among them)."""
    rng = np.random.default_rng(1000 * H_ + W + seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (n, H_, W, 3), dtype=np.uint8)
    return rng.integers(0, 2 ** 32, (n, H_, W, 3), dtype=np.uint32).view(np.float32)
