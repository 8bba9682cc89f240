"""Test-time-augmentation views on the device: fav_op_views against tests/views_ref.py, and a handle with views set against
the same handle, views off, run on the reference's view frames.

Everything here is an equality of bits.  The views are data movement, so the op's output must be the reference's bytes; a
call with views runs the unchanged forward pass on [view][frame] frames, so its logits must be the bits of a views-off call
on the reference's A * n view frames (the same number of frames: the same schedule), and every head output must be the bits
of the corresponding fav_op_head* on those logits with T = T_head * A.  (The heads read num_classes values a row whatever
the row stride, which tests/test_gpu_calibration.py already relies on.)

Shapes: one pixel, one row, sizes with no full group of four pixels, odd sizes, one more and one less than the 32-pixel tile
of the transposed kernel, the tile itself, and one 224 x 224 frame; 1 and 3 frames.  Shifts reach 2 * size + 1, beyond one
period 2 (size - 1) of reflect-101.

One case of the issue is restated: a ViT-tiny handle of 24 x 32 cannot exist (the patch is 16 pixels), so the refusal of a
transpose on a handle with in_h != in_w is checked on 16 x 32."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import views_ref as R  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, synth, views, weights  # noqa: E402
from failure_aware_vision_amd.conformal import Conformal  # noqa: E402

GUARD = 64
SIZES = ((1, 1), (1, 5), (3, 4), (7, 9), (8, 8), (13, 13), (31, 31), (32, 32), (33, 33))
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def c_views(vs):
    vs = [R.as_dict(v) for v in vs]
    return (_lib.FavView * max(1, len(vs)))(*[_lib.FavView(v["flip_x"], v["flip_y"], v["transpose"], v["dy"], v["dx"], v["border"])
                                              for v in vs]), len(vs)


def frames_of(n, H, W, dtype, seed=0):
    """uint8: random bytes.  float32: random BIT PATTERNS (NaNs of both kinds, infinities and subnormals among them)."""
    rng = np.random.default_rng(1000 * H + W + seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    return rng.integers(0, 2 ** 32, (n, H, W, 3), dtype=np.uint32).view(np.float32)


def run_op(lib, frames, vs, in_off=0, out_off=0):
    """fav_op_views on `frames` placed in_off bytes into a buffer, writing out_off bytes behind a guard -> (status, the
    output's bytes as frames.dtype [A, n, H, W, 3], guards untouched?)."""
    n, H, W, _ = frames.shape
    arr, A = c_views(vs)
    raw = np.ascontiguousarray(frames).view(np.uint8).ravel()
    inbuf = torch.zeros(raw.size + 32, dtype=torch.uint8, device="cuda")
    inbuf[in_off:in_off + raw.size] = torch.from_numpy(raw).cuda()
    nout = raw.size * A
    outbuf = torch.full((GUARD + 16 + nout + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert inbuf.data_ptr() % 16 == 0 and outbuf.data_ptr() % 16 == 0
    lo = GUARD + out_off
    st = lib.fav_op_views(inbuf.data_ptr() + in_off, outbuf.data_ptr() + lo, n, H, W,
                          _lib.LAYOUT_NHWC_U8 if frames.dtype == np.uint8 else _lib.LAYOUT_NHWC_F32, arr, A,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = outbuf.cpu().numpy()
    guards = bool((host[:lo] == 0xA5).all() and (host[lo + nout:] == 0xA5).all())
    return st, host[lo:lo + nout].copy().view(frames.dtype).reshape(A, n, H, W, 3), guards


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def shift_values(size):
    return (0, 1, -1, size - 1, -(size - 1), size, -size, 2 * size + 1, -(2 * size + 1))


def all_views(H, W):
    """Every flag combination (a transpose on square frames only) x the three borders x 25 shift pairs: each shift value
    alone along y, alone along x, and paired with another along the other axis."""
    sy, sx = shift_values(H), shift_values(W)
    pairs = [(d, 0) for d in sy] + [(0, d) for d in sx[1:]] + [(sy[k], sx[(k + 4) % 9]) for k in range(1, 9)]
    out = []
    for fx, fy, tr in itertools.product((0, 1), repeat=3):
        if tr and H != W:
            continue
        for border in (R.REFLECT101, R.REPLICATE, R.ZERO):
            out += [R.V(fx, fy, tr, dy, dx, border) for dy, dx in pairs]
    return out


def chunks(vs):
    """1, 5 and 64 views a call, then 64 a call."""
    sizes, i = [1, 5, 64], 0
    while i < len(vs):
        k = sizes.pop(0) if sizes else 64
        yield vs[i:i + k]
        i += k


# ---- fav_op_views ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.uint8, np.float32), ids=("u8", "f32"))
@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_op_bit_exact(lib, size, n, dtype):
    H, W = size
    frames = frames_of(n, H, W, dtype)
    vs = all_views(H, W)
    assert len(vs) == (600 if H == W else 300)
    for part in chunks(vs):
        st, got, guards = run_op(lib, frames, part)
        assert st == 0 and guards
        want = R.apply_views(frames, part)
        if not same_bits(got, want):
            bad = [v for a, v in enumerate(part) if not same_bits(got[a], want[a])]
            raise AssertionError(f"{len(bad)} of {len(part)} views differ, the first: {bad[0]}")


@pytest.mark.parametrize("dtype", (np.uint8, np.float32), ids=("u8", "f32"))
def test_op_one_large_frame(lib, dtype):
    frames = frames_of(1, 224, 224, dtype)
    vs = views.d4() + views.shifts(2) + [R.V(1, 0, 0, 223, -1, R.ZERO), R.V(0, 1, 1, -224, 449, R.REFLECT101),
                                         R.V(1, 1, 1, 1, -223, R.REPLICATE), R.V(0, 0, 0, -449, 224, R.REFLECT101)]
    st, got, guards = run_op(lib, frames, vs)
    assert st == 0 and guards and same_bits(got, R.apply_views(frames, vs))


@pytest.mark.parametrize("dtype", (np.uint8, np.float32), ids=("u8", "f32"))
def test_op_buffer_offsets(lib, dtype):
    """uint8 buffers 1, 2 and 3 bytes off a 16-byte boundary, fp32 buffers 4, 8 and 12 bytes off, input and output
    independently: the head and tail groups, the shifted dword loads and the fp32 rows that are not 16-byte aligned."""
    esz = np.dtype(dtype).itemsize
    vs = [R.V(), R.V(flip_x=1), R.V(dx=1), R.V(flip_x=1, dx=-2, dy=1, border=R.ZERO), R.V(transpose=1),
          R.V(flip_y=1, transpose=1, dx=3, border=R.REPLICATE)]
    for H, W in ((5, 5), (9, 9), (33, 33), (40, 40)):
        frames = frames_of(2, H, W, dtype, seed=7)
        want = R.apply_views(frames, vs)
        for in_off, out_off in itertools.product((0, esz, 2 * esz, 3 * esz), repeat=2):
            st, got, guards = run_op(lib, frames, vs, in_off, out_off)
            assert st == 0 and guards and same_bits(got, want), (H, W, in_off, out_off)


def test_op_copies_nan_payloads_and_negative_zero(lib):
    words = np.array([0x7FC12345, 0xFFA00001, 0x7F800001, 0x80000000, 0x00000001, 0xFF800000, 0x7FFFFFFF, 0x80000001,
                      0x3F800000, 0x00000000, 0xFFFFFFFF, 0x7FC00000], np.uint32)
    frames = np.resize(words, 2 * 4 * 6 * 3).reshape(2, 4, 6, 3).view(np.float32)
    vs = [R.V(), R.V(flip_x=1, flip_y=1), R.V(dx=1, border=R.REPLICATE), R.V(dy=-1)]
    st, got, guards = run_op(lib, frames, vs)
    assert st == 0 and guards
    assert np.array_equal(got[0].view(np.uint32), frames.view(np.uint32))          # the identity keeps every payload
    assert same_bits(got, R.apply_views(frames, vs))
    sq = np.resize(words, 1 * 5 * 5 * 3).reshape(1, 5, 5, 3).view(np.float32)
    st, got, guards = run_op(lib, sq, [R.V(transpose=1)])
    assert st == 0 and guards and np.array_equal(got[0].view(np.uint32), sq.view(np.uint32).transpose(0, 2, 1, 3))
    z = run_op(lib, sq, [R.V(dx=5, border=R.ZERO)])[1]
    assert (z.view(np.uint32) == 0).all()                                          # outside the frame: +0.0f


def test_op_refusals_launch_nothing(lib):
    frames = torch.full((2 * 8 * 8 * 3 * 4 + 64,), 7, dtype=torch.uint8, device="cuda")
    out = torch.full((65 * 2 * 8 * 8 * 3 * 4 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    one, _ = c_views([R.V()])
    many, _ = c_views([R.V()] * 65)
    tr, _ = c_views([R.V(transpose=1)])
    bad, _ = c_views([R.V(border=3)])
    f, o = frames.data_ptr(), out.data_ptr()
    U8, F32 = _lib.LAYOUT_NHWC_U8, _lib.LAYOUT_NHWC_F32
    cases = [("65 views", (f, o, 2, 8, 8, U8, many, 65), "n_views=65"), ("no views", (f, o, 2, 8, 8, U8, one, 0), "n_views=0"),
             ("null frames", (None, o, 2, 8, 8, U8, one, 1), "null"), ("null out", (f, None, 2, 8, 8, U8, one, 1), "null"),
             ("null views", (f, o, 2, 8, 8, U8, None, 1), "NULL"), ("n 0", (f, o, 0, 8, 8, U8, one, 1), "at least 1"),
             ("H 0", (f, o, 2, 0, 8, U8, one, 1), "at least 1"), ("layout", (f, o, 2, 8, 8, 2, one, 1), "layout"),
             ("transpose 8x4", (f, o, 2, 8, 4, U8, tr, 1), "transpose needs H == W"), ("border", (f, o, 2, 8, 8, U8, bad, 1), "border=3"),
             ("f32 frames + 2", (f + 2, o, 2, 8, 8, F32, one, 1), "aligned"), ("f32 out + 1", (f, o + 1, 2, 8, 8, F32, one, 1), "aligned"),
             # overlaps: out inside frames, frames inside out, the last byte of one on the first of the other
             ("out == frames", (f, f, 2, 8, 8, U8, one, 1), "overlaps"), ("out in frames", (f, f + 383, 2, 8, 8, U8, one, 1), "overlaps"),
             ("frames in out", (o + 384 * 3, o, 2, 8, 8, U8, many, 5), "overlaps"),
             ("out end on frames", (o + 384 * 2 - 1, o, 2, 8, 8, U8, many, 2), "overlaps")]
    for why, args, text in cases:
        st = lib.fav_op_views(*args, stream)
        torch.cuda.synchronize()
        msg = lib.fav_last_error(None).decode()
        assert st == 1 and "fav_op_views" in msg and text in msg, (why, msg)
        assert bool((out == 0xA5).all()) and bool((frames == 7).all()), why
    # touching ranges do not overlap
    assert lib.fav_op_views(o + 384 * 2, o, 2, 8, 8, U8, many, 2, stream) == 0
    assert lib.fav_op_views(o, o + 384, 2, 8, 8, U8, one, 1, stream) == 0
    torch.cuda.synchronize()


def test_apply_matches_the_op(lib):
    frames = frames_of(3, 7, 7, np.uint8)
    vs = views.product(views.d4(), views.shifts(1, "zero"))[:11]
    got = views.apply(torch.from_numpy(frames).cuda(), vs)
    assert tuple(got.shape) == (11, 3, 7, 7, 3) and got.dtype == torch.uint8
    assert same_bits(got.cpu().numpy(), R.apply_views(frames, vs))
    f32 = frames_of(2, 4, 6, np.float32)
    assert same_bits(views.apply(torch.from_numpy(f32).cuda(), views.hflip()).cpu().numpy(), R.apply_views(f32, views.hflip()))
    with pytest.raises(_lib.FavError, match="fav_op_views"):
        views.apply(torch.from_numpy(f32).cuda(), views.d4())
    with pytest.raises(ValueError):
        views.apply(torch.from_numpy(f32).cuda().double(), views.hflip())


# ---- a handle with views -----------------------------------------------------------------------------------------------
MAX_BATCH, N = 32, 3
VIEWS = views.product(views.d4(), views.shifts(1))[:6] + [views.View(dy=-2, dx=3, border="zero"),
                                                          views.View(flip_x=True, transpose=True, dy=1, border="replicate")]
A = len(VIEWS)
ARCHS = ("resnet18_cifar", "vit_tiny", "ensemble")
CP = Conformal(kind="aps", randomized=True, qhat=0.9, seed=77)
TEMPS = (0.5, 0.8, 1.0, 1.7, 4.0)


def make_backend(arch, **kw):
    if arch == "vit_tiny":
        blob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
        return Backend("vit_tiny", blob, max_batch=MAX_BATCH, **kw), 64
    if arch == "ensemble":
        blobs = [weights.make_synthetic("resnet18_cifar", seed=s)[0] for s in (1, 2, 3)]
        return Backend("resnet18_cifar", blobs, max_batch=MAX_BATCH, **kw), 32
    blob, _ = weights.make_synthetic("resnet18_cifar", seed=1)
    return Backend("resnet18_cifar", blob, max_batch=MAX_BATCH, **kw), 32


@pytest.fixture(scope="module", params=ARCHS)
def handle(request):
    """(backend with temperature 1.3 and tau 0.4, its frames uint8 [N, S, S, 3], the reference's A * N view frames)."""
    be, S = make_backend(request.param, temperature=1.3, tau=0.4, conf_kind="entropy")
    frames = synth.synthetic_frames_u8(N, S, S, seed=21)
    ref = R.apply_views(frames, VIEWS).reshape(A * N, S, S, 3)
    yield be, frames, ref
    be.close()


def all_outputs(be, dev, first=1000):
    """Every head of the handle on `dev` -> dict of numpy arrays (the records as int32)."""
    out = {}
    lab, conf, fail, score = be.classify_detect(dev, first)
    out.update(labels=lab, conf=conf, fail=fail, score=score)
    out["logits"] = be.logits()
    out["records"] = be.classify_records(dev, first)
    unc = torch.full((dev.shape[0], 18), -7, dtype=torch.int32, device="cuda")
    r = be.classify_uncertainty(dev, first, out=unc)
    out.update(unc=unc, unc_fail=r["fail"], unc_score=r["score"])
    sets = torch.full((dev.shape[0], 40), -7, dtype=torch.int32, device="cuda")
    r = be.classify_sets(dev, CP, first, out=sets)
    out.update(sets=sets, sets_fail=r["fail"])
    y = torch.arange(dev.shape[0], dtype=torch.int32, device="cuda") % be.cfg.num_classes
    out["cells"] = be.calibration_sweep(dev, y, TEMPS, first)
    out["cscores"] = be.conformal_scores(dev, y, CP, first)
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits_equal(a, b):
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def test_handle_logits_and_heads(lib, handle):
    be, frames, ref = handle
    dev = torch.from_numpy(frames).cuda()
    Cc, T_head = int(be.cfg.num_classes), be.T
    off = all_outputs(be, dev)                                                     # views off, before
    assert off["logits"].shape == (T_head, N, Cc)
    be.set_views(VIEWS)
    assert be.views == tuple(VIEWS) and be.T == T_head * A and be.frames_per_call == MAX_BATCH // A
    n_out = C.c_int32()
    back = (_lib.FavView * A)()
    _lib.check(lib.fav_get_views(be._h, back, A, C.byref(n_out)), be._h)
    assert n_out.value == A and [views.View.from_c(v) for v in back] == VIEWS
    on = all_outputs(be, dev)
    T = T_head * A
    assert on["logits"].shape == (T, N, Cc)
    # the logits: a views-off call on the reference's A * N view frames, sample s = m * A + a
    be.set_views(None)
    assert be.views == () and be.T == T_head
    be.classify(torch.from_numpy(ref).cuda())
    want = be.logits().cpu().numpy()
    assert want.shape == (T_head, A * N, Cc)
    want = want.reshape(T_head, A, N, Cc).reshape(T, N, Cc)
    assert np.array_equal(on["logits"].view(np.int32), want.view(np.int32))
    # the heads: fav_op_head* on those logits with T = T_head * A
    ld = (Cc + 3) // 4 * 4
    lg = torch.zeros((T, N, ld), dtype=torch.float32, device="cuda")
    lg[:, :, :Cc] = torch.from_numpy(want).cuda()
    temp, kind, tau = be.cfg.temperature, be.cfg.conf_kind, be.cfg.tau
    lab = torch.empty(N, dtype=torch.int32, device="cuda")
    conf, score = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    fail = torch.empty(N, dtype=torch.uint8, device="cuda")
    _lib.check(lib.fav_op_head(lg.data_ptr(), T, N, Cc, ld, temp, kind, tau, lab.data_ptr(), conf.data_ptr(), fail.data_ptr(),
                               score.data_ptr(), None))
    unc = torch.full((N, 18), -9, dtype=torch.int32, device="cuda")
    ufail, uscore = torch.empty(N, dtype=torch.uint8, device="cuda"), torch.empty(N, device="cuda")
    _lib.check(lib.fav_op_head_uncertainty(lg.data_ptr(), T, N, Cc, ld, temp, kind, tau, unc.data_ptr(), ufail.data_ptr(),
                                           uscore.data_ptr(), None))
    sets = torch.full((N, 40), -9, dtype=torch.int32, device="cuda")
    sfail = torch.empty(N, dtype=torch.uint8, device="cuda")
    y = torch.arange(N, dtype=torch.int32, device="cuda") % Cc
    cscores = torch.empty(N, device="cuda")
    _lib.check(lib.fav_op_head_sets(lg.data_ptr(), T, N, Cc, ld, temp, kind, tau, 1000, CP.to_c(), y.data_ptr(), cscores.data_ptr(),
                                    sets.data_ptr(), sfail.data_ptr(), None, None))
    t = np.asarray(TEMPS, np.float32)
    cells = torch.full((N, t.size, 4), -9, dtype=torch.int32, device="cuda")
    _lib.check(lib.fav_op_head_sweep(lg.data_ptr(), T, N, Cc, ld, t.ctypes.data_as(C.POINTER(C.c_float)), t.size, kind, y.data_ptr(),
                                     cells.data_ptr(), None))
    torch.cuda.synchronize()
    ops = dict(labels=lab, conf=conf, fail=fail, score=score, unc=unc, unc_fail=ufail, unc_score=uscore, sets=sets, sets_fail=sfail,
               cells=cells, cscores=cscores)
    for k, v in ops.items():
        assert np.array_equal(on[k].view(np.uint8), v.cpu().numpy().view(np.uint8)), k
    assert np.array_equal(on["records"][:, 0], on["labels"]) and np.array_equal(on["records"][:, 1], on["conf"].view(np.int32))
    assert not np.array_equal(on["logits"][0], on["logits"][1])                    # member 0 under views 0 and 1
    # views off again: every result is the one from before
    assert bits_equal(all_outputs(be, dev), off)
    # a single identity view: the bits of views off
    be.set_views(views.identity())
    assert be.T == T_head and bits_equal(all_outputs(be, dev), off)
    be.set_views(None)


# ---- views at odd frame sizes, against the oracle -----------------------------------------------------------------------
ODD_VIEWS = {
    # 31 x 45: every stage of ResNet-18 is odd along one axis at least (31 x 45, 16 x 23, 8 x 12, 4 x 6), and no view may swap
    # the axes.  The mirror images, then one shift under each border rule - beyond the frame's edge on both axes
    (31, 45): [views.View(), views.View(flip_x=True), views.View(flip_y=True), views.View(dy=3, dx=-5, border="reflect101"),
               views.View(dy=-2, dx=4, border="replicate"), views.View(dy=5, dx=7, border="zero")],
    # 33 x 33: one pixel more than the transposed kernel's 32-pixel tile
    (33, 33): [views.View(), views.View(transpose=True), views.View(flip_x=True, transpose=True, dy=1, border="replicate")],
}


@pytest.mark.parametrize("hw", list(ODD_VIEWS), ids=ids)
def test_views_at_an_odd_frame_size_against_the_oracle(hw):
    """The handle's logits under views are the oracle's (the bit-exact model of the production mode) on views_ref's expanded
    frames: sample a of frame i is view a of frame i - which pins the view kernel's H x W indexing and the forward pass at
    this size in one comparison."""
    from oracle import fav_oracle as O
    vs = ODD_VIEWS[hw]
    blob, _ = weights.make_synthetic("resnet18_cifar", seed=1)
    frames = synth.synthetic_frames_u8(N, hw[0], hw[1], seed=21)
    expanded = R.apply_views(frames, vs)                                            # [A, N, H, W, 3]
    assert all(not np.array_equal(expanded[0], expanded[a]) for a in range(1, len(vs)))
    want = O.classify(O.parse_blob(blob), expanded.reshape(len(vs) * N, hw[0], hw[1], 3), O.ClassifyConfig(exact="mfma"),
                      return_logits=True)[2]
    want = want.reshape(len(vs), N, -1)
    be = Backend("resnet18_cifar", blob, in_hw=hw, max_batch=MAX_BATCH, views=vs)
    try:
        assert be.T == len(vs)
        for dev in (torch.from_numpy(frames).cuda(), torch.from_numpy(frames.astype(np.float32) / np.float32(255.0)).cuda()):
            if dev.dtype == torch.float32:                                          # fp32 frames: the oracle on the same pixels
                want = O.classify(O.parse_blob(blob), R.apply_views(dev.cpu().numpy(), vs).reshape(len(vs) * N, hw[0], hw[1], 3),
                                  O.ClassifyConfig(exact="mfma"), return_logits=True)[2].reshape(len(vs), N, -1)
            be.classify(dev)
            got = be.logits().cpu().numpy()
            assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), str(dev.dtype)
            assert not np.array_equal(got[0], got[1])
    finally:
        be.close()


def test_handle_host_frames_and_f32(handle):
    be, frames, _ = handle
    be.set_views(VIEWS)
    dev = torch.from_numpy(frames).cuda()
    d = [x.cpu().numpy() for x in be.classify_detect(dev, 5)]
    h = be.classify_detect(frames, 5)                                              # numpy in: fav_classify_host
    assert all(isinstance(x, np.ndarray) for x in h)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(d, h))
    # fp32 frames go through the fp32 view kernel (and grow the view buffer): the logits of the reference's fp32 view frames
    f32 = (frames.astype(np.float32) * np.float32(1 / 255)).astype(np.float32)
    be.classify(torch.from_numpy(f32).cuda())
    got = be.logits().cpu().numpy()
    be.set_views(None)
    ref = R.apply_views(f32, VIEWS).reshape(A * N, *f32.shape[1:])
    be.classify(torch.from_numpy(ref).cuda())
    want = be.logits().cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.reshape(-1, A, N, want.shape[2]).reshape(got.shape).view(np.int32))


def test_views_give_the_uncertainty_outputs_something_to_say(handle):
    be, frames, _ = handle
    noise = np.random.default_rng(5).integers(0, 256, (4,) + frames.shape[1:], dtype=np.uint8)
    dev = torch.from_numpy(noise).cuda()
    if be.T == 1:                                                                  # a single pass: nothing to disagree
        r = be.classify_uncertainty(dev)
        assert bool((r["mutual_info"] == 0).all()) and bool((r["agreement"] == 1).all()) and bool((r["prob_std"] == 0).all())
    be.set_views(VIEWS)
    r = {k: v.cpu().numpy() for k, v in be.classify_uncertainty(dev).items()}
    be.set_views(None)
    print("views:", be.arch, "mutual_info", r["mutual_info"], "agreement", r["agreement"], "prob_std", r["prob_std"])
    assert (r["mutual_info"] > 0).any() and (r["agreement"] < 1).any() and (r["prob_std"] > 0).any()


def test_batched_methods_use_frames_per_call(handle):
    be, frames, _ = handle
    S = frames.shape[1]
    many = synth.synthetic_frames_u8(10, S, S, seed=9)
    dev = torch.from_numpy(many).cuda()
    y = torch.arange(10, dtype=torch.int32, device="cuda") % be.cfg.num_classes
    be.set_views(VIEWS)
    per = be.frames_per_call
    assert per == 4
    cells = be.calibration_sweep(dev, y, TEMPS, first_index=50)
    scores = be.conformal_scores(dev, y, CP, first_index=50)
    lab, conf = be._detect_batched(dev, 50)
    parts_c, parts_s, parts_l = [], [], []
    for b in range(0, 10, per):
        e = min(10, b + per)
        parts_c.append(be.calibration_sweep(dev[b:e], y[b:e], TEMPS, first_index=50 + b))
        parts_s.append(be.conformal_scores(dev[b:e], y[b:e], CP, first_index=50 + b))
        parts_l.append(be.classify(dev[b:e], 50 + b)[0])
    assert torch.equal(cells, torch.cat(parts_c)) and torch.equal(scores.view(torch.int32), torch.cat(parts_s).view(torch.int32))
    assert np.array_equal(lab, torch.cat(parts_l).cpu().numpy())
    fit = be.calibrate_temperature(dev, y)                                         # the sweep's logits are kept per batch
    assert fit.temperature > 0
    with pytest.raises(ValueError, match="logits_budget_bytes"):
        be.calibrate_temperature(dev, y, logits_budget_bytes=4 * be.T * 10 * ((be.cfg.num_classes + 3) // 4 * 4) - 1)
    be.set_views(None)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_handle_refusals(lib):
    be, S = make_backend("resnet18_cifar")
    dev = torch.from_numpy(synth.synthetic_frames_u8(5, S, S, seed=2)).cuda()
    before = [x.cpu().numpy() for x in be.classify_detect(dev)]
    be.set_views(VIEWS)
    with pytest.raises(_lib.FavError) as e:                                       # 5 x 8 > 32
        be.classify(dev)
    assert e.value.status == 1 and all(t in str(e.value) for t in ("n=5", "n_views=8", "max_batch=32"))
    for call in (lambda: be.classify_records(dev), lambda: be.classify_uncertainty(dev), lambda: be.classify_sets(dev, CP),
                 lambda: be.classify_detect(dev.cpu().numpy())):
        with pytest.raises(_lib.FavError, match="n_views=8"):
            call()
    be.classify(dev[:4])                                                           # 4 x 8 = 32 fits
    # the views are checked by the setter, and a refused setter leaves the handle as it was
    for bad, text in (([views.View(dy=70000)], "dy=70000"), ([views.View()] * 65, "n_views=65"), ([views.View()] * 33, "max_batch=32")):
        with pytest.raises(_lib.FavError, match=text):
            be.set_views(bad)
        assert be.views == tuple(VIEWS)
    # mutual information needs two samples
    be.set_views(None)
    with pytest.raises(_lib.FavError, match="fav_set_conf_kind"):
        be.set_conf_kind("mutual_info")
    be.set_views(views.identity())
    with pytest.raises(_lib.FavError, match="fav_set_conf_kind"):
        be.set_conf_kind("mutual_info")
    assert lib.fav_set_conf_kind(be._h, 3) == 1 and lib.fav_set_conf_kind(be._h, -1) == 1
    be.set_views(views.hflip())
    be.set_conf_kind("mutual_info")                                                # two views: accepted
    lab, conf = be.classify(dev)
    lg = be.logits()
    assert tuple(lg.shape) == (2, 5, 10)
    ld = torch.zeros((2, 5, 12), device="cuda")
    ld[:, :, :10] = lg
    l2, c2 = torch.empty(5, dtype=torch.int32, device="cuda"), torch.empty(5, device="cuda")
    _lib.check(lib.fav_op_head(ld.data_ptr(), 2, 5, 10, 12, 1.0, _lib.CONF_MUTUAL_INFO, 0.5, l2.data_ptr(), c2.data_ptr(), None, None, None))
    torch.cuda.synchronize()
    assert torch.equal(lab, l2) and torch.equal(conf.view(torch.int32), c2.view(torch.int32))
    for off in (None, views.identity()):
        with pytest.raises(_lib.FavError, match="change the kind first"):
            be.set_views(off)
        assert be.views == tuple(views.hflip())
    be.set_conf_kind("entropy")
    be.set_views(None)
    be.set_conf_kind("max_softmax")
    after = [x.cpu().numpy() for x in be.classify_detect(dev)]
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, after))
    be.close()
    # the constructor: mutual information over views alone
    be, _ = make_backend("resnet18_cifar", conf_kind="mutual_info", views=views.hflip())
    assert be.cfg.conf_kind == _lib.CONF_MUTUAL_INFO and be.T == 2 and be.views == tuple(views.hflip())
    assert torch.equal(be.classify(dev)[1].view(torch.int32), conf.view(torch.int32))
    be.close()
    with pytest.raises(_lib.FavError):
        make_backend("resnet18_cifar", conf_kind="mutual_info", views=views.identity())


def test_mc_dropout_handles_are_refused():
    blob, _ = weights.make_synthetic("resnet18_cifar", seed=1)
    be = Backend("resnet18_cifar", blob, max_batch=8, n_samples=3, dropout_policy="all_blocks", dropout_p=0.1, seed=4)
    with pytest.raises(_lib.FavError) as e:
        be.set_views(views.hflip())
    assert e.value.status == 6 and "MC-Dropout" in str(e.value) and be.views == ()      # FAV_ERR_UNSUPPORTED
    be.set_views(None)                                                             # off stays allowed
    be.close()
    be = Backend("resnet18_cifar", blob, max_batch=8, n_samples=3, dropout_policy="all_blocks", dropout_p=0.001)
    be.set_views(views.hflip())                                                    # round(256 p) = 0: no masks are drawn
    assert be.T == 2
    be.close()


def test_transpose_needs_a_square_handle():
    blob, _ = weights.make_synthetic_vit("vit_tiny", seed=3, in_hw=(16, 32))
    be = Backend("vit_tiny", blob, max_batch=32, in_hw=(16, 32))
    with pytest.raises(_lib.FavError) as e:
        be.set_views(views.d4())
    assert e.value.status == 1 and "transpose needs H == W" in str(e.value) and "16x32" in str(e.value)
    be.set_views(views.product(views.hflip(), views.shifts(1)))                    # the straight views are fine
    frames = synth.synthetic_frames_u8(3, 16, 32, seed=4)
    be.classify(torch.from_numpy(frames).cuda())
    got = be.logits().cpu().numpy()
    vs = list(be.views)
    be.set_views(None)
    be.classify(torch.from_numpy(R.apply_views(frames, vs).reshape(-1, 16, 32, 3)).cuda())
    want = be.logits().cpu().numpy()
    assert len(vs) == 10 and got.shape == (10, 3, be.cfg.num_classes) and want.shape == (1, 30, be.cfg.num_classes)
    assert np.array_equal(got.view(np.int32), want.reshape(got.shape).view(np.int32))
    be.close()
