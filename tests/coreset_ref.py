"""The numpy restatement of greedy coreset selection as include/fav.h defines it beside fav_check_coreset: float32 operations
only, in the stated order, min and max on values, the lowest row on a tie.  tests/test_coreset_host.py checks its properties
on the CPU; tests/test_gpu_coreset.py asks the device for its dwords."""
import numpy as np

F32 = np.float32
_BLOCK = 4096          # rows a call of sims() holds as float32 at a time


def bits_to_f32(bits) -> np.ndarray:
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(F32)


def f32_to_bf16_bits(x) -> np.ndarray:
    """finite float32 -> bf16 bit patterns, round to nearest even."""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def sims(bits, c: int) -> np.ndarray:
    """float32 [N]: rows . rows[c].  64 chains, element j in chain (j / 8) % 64, a chain acc = acc + a[j] * b[j] over its elements
    in ascending j from +0, then s[l] = s[l] + s[l + w] for w = 32 .. 1.  Elements past D are +0 products: adding them changes
    no bit, since a chain that starts at +0 never holds -0."""
    bits = np.asarray(bits, np.uint16)
    N, D = bits.shape
    steps = -(-D // 512)
    b = np.zeros(steps * 512, F32)
    b[:D] = bits_to_f32(bits[c])
    out = np.empty(N, F32)
    for r0 in range(0, N, _BLOCK):
        a = np.zeros((min(_BLOCK, N - r0), steps * 512), F32)
        a[:, :D] = bits_to_f32(bits[r0:r0 + _BLOCK])
        prod = (a * b).reshape(a.shape[0], steps, 64, 8)             # exact: two bf16
        acc = np.zeros((a.shape[0], 64), F32)
        for s in range(steps):
            for e in range(8):
                acc = acc + prod[:, s, :, e]
        w = 32
        while w >= 1:
            acc = acc[:, :w] + acc[:, w:2 * w]
            w //= 2
        out[r0:r0 + _BLOCK] = acc[:, 0]
    return out


def dist(sim) -> np.ndarray:
    """max(2 - 2 * sim, 0), the product and the difference rounded on their own."""
    return np.maximum(F32(2.0) - F32(2.0) * np.asarray(sim, F32), F32(0.0)).astype(F32)


def select(bits, M: int, start: int, sims_fn=sims):
    """-> (order int32 [M], radius float32 [M + 1]).  ``sims_fn(bits, c)``: the similarities of every row to row c."""
    bits = np.asarray(bits, np.uint16)
    N = bits.shape[0]
    assert 1 <= M <= N and 0 <= start < N
    order = np.empty(M, np.int32)
    radius = np.empty(M + 1, F32)
    order[0], radius[0] = start, np.inf
    mind = np.full(N, np.inf, F32)
    taken = np.zeros(N, bool)
    for t in range(1, M + 1):
        c = int(order[t - 1])
        taken[c] = True
        mind = np.minimum(mind, dist(sims_fn(bits, c)))
        free = np.flatnonzero(~taken)
        if free.size == 0:
            radius[t] = 0.0
            assert t == M
            continue
        best = free[np.argmax(mind[free])]                           # argmax takes the first, free ascends: the lowest row
        radius[t] = mind[best]
        if t < M:
            order[t] = best
    return order, radius
