"""Class activation maps on the device: fav_op_cam and fav_op_cam_heatmap against tests/cam_ref.py, the map tap against the
feature tap and the logits, and the Backend methods end to end.

Bits are compared with the reference throughout (R.same_bits: a NaN counts as equal to any NaN).  The contract (include/fav.h
beside fav_cam_record) fixes every product and every sum, so maps and records must be the reference's dwords.

Shapes of the op: the whole product S in {1, 3}, n in {1, 5}, (Hf, Wf) in {(1, 1), (4, 4), (7, 7), (8, 10)}, C in {512, 2048},
K in {1, 5, 8}.  The kernel runs 16 waves a block and a wave a cell, with the loads of four 512-channel steps ahead of their
chain: 1, 49 and 80 cells are no multiple of 16, S * C / 512 = 1 and 3 are no multiple of 4, and K = 1 takes another
instantiation than K = 5 and 8.  Every case has guard bytes around its maps and records."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import cam_ref as R  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, synth, views, weights  # noqa: E402
from failure_aware_vision_amd.cam import unpack_cam_records  # noqa: E402
from oracle import fav_oracle as O  # noqa: E402

GUARD = 64
FILL = 0x5A
NC = 37          # classes of the op tests


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(nbytes):
    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf


def guards_ok(buf, nbytes):
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == FILL).all() and (host[GUARD + nbytes:] == FILL).all())


def run_cam(lib, xb, wb, bias, classes, hf, wf, n_classes=NC, **over):
    """fav_op_cam -> (status, maps float32 [n, K, HW], records int32 [n, K, 8], guards untouched?, outputs untouched?).
    over: sizes to pass instead of the arrays' own (S, n, Hf, Wf, C, ldw, n_classes, K), and null = names passed as NULL."""
    S, n, HW, Cc = xb.shape
    classes = np.asarray(classes, np.int32).reshape(n, -1)
    K = classes.shape[1]
    t = dict(maps=dev(xb.view(np.int16)), w=dev(wb.view(np.int16)), bias=dev(np.asarray(bias, np.float32)), classes=dev(classes))
    cam_bytes, rec_bytes = n * K * HW * 4, n * K * 32
    cam, rec = guarded(cam_bytes), guarded(rec_bytes)
    null = over.pop("null", ())
    ptr = {k: (None if k in null else v.data_ptr()) for k, v in t.items()}
    a = dict(S=S, n=n, Hf=hf, Wf=wf, C=Cc, ldw=wb.shape[1], n_classes=n_classes, K=K)
    a.update(over)
    st = lib.fav_op_cam(ptr["maps"], a["S"], a["n"], a["Hf"], a["Wf"], a["C"], ptr["w"], a["ldw"], ptr["bias"], a["n_classes"],
                        ptr["classes"], a["K"], None if "cam" in null else cam.data_ptr() + GUARD,
                        None if "rec" in null else rec.data_ptr() + GUARD, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ch, rh = cam.cpu().numpy()[GUARD:GUARD + cam_bytes], rec.cpu().numpy()[GUARD:GUARD + rec_bytes]
    untouched = bool((ch == FILL).all() and (rh == FILL).all())
    return (st, ch.copy().view(np.float32).reshape(n, K, HW), rh.copy().view(np.int32).reshape(n, K, 8),
            guards_ok(cam, cam_bytes) and guards_ok(rec, rec_bytes), untouched)


def problem(seed, S, n, HW, Cc, ldw=None):
    """ReLU-like maps (half the values zero), signed weights -> (x_bits, w_bits [NC, ldw], bias)."""
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((S, n, HW, Cc)), 0.0).astype(np.float32)
    w = (rng.standard_normal((NC, ldw or Cc)) * 0.05).astype(np.float32)
    return R.f32_to_bf16_bits(x), R.f32_to_bf16_bits(w), rng.standard_normal(NC).astype(np.float32)


def classes_for(rng, n, K):
    """Random classes; from K = 5 on: a duplicate in every row, and a -1 and an n_classes beside the valid ones."""
    c = rng.integers(0, NC, (n, K))
    if K >= 5:
        c[:, 1] = c[:, 0]
        c[:, 2] = -1
        c[:, K - 1] = NC
        c[0, 3] = NC + 1000
    return c


def check_against_reference(got, xb, wb, bias, classes, Wf, n_classes=NC):
    st, M, rec, guards, _ = got
    assert st == 0 and guards
    Mr, rr = R.cam(xb, wb, bias, classes, n_classes, Wf)
    assert R.same_bits(M, Mr)
    f = (1, 2, 4, 5)
    assert np.array_equal(np.delete(rec, f, axis=2), np.delete(rr, f, axis=2))
    assert R.same_bits(rec[..., f].view(np.float32), rr[..., f].view(np.float32))


@pytest.mark.parametrize("K", [1, 5, 8])
@pytest.mark.parametrize("Cc", [512, 2048])
@pytest.mark.parametrize("hw", [(1, 1), (4, 4), (7, 7), (8, 10)])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("S", [1, 3])
def test_op_cam_matches_the_reference(lib, S, n, hw, Cc, K):
    Hf, Wf = hw
    seed = ((S * 10 + n) * 100 + Hf * Wf) * 10000 + Cc + K
    ldw = Cc + (8 if (n + K) % 2 else 0)                  # ldw > C in half the cases
    xb, wb, bias = problem(seed, S, n, Hf * Wf, Cc, ldw)
    classes = classes_for(np.random.default_rng(seed + 1), n, K)
    check_against_reference(run_cam(lib, xb, wb, bias, classes, Hf, Wf), xb, wb, bias, classes, Wf)


def test_op_cam_all_negative_map_equal_peaks_and_a_nan(lib):
    S, n, Hf, Wf, Cc = 3, 2, 7, 7, 1024
    xb, wb, bias = problem(5, S, n, Hf * Wf, Cc, Cc + 16)
    w = R.bf16_bits_to_f32(wb).copy()
    w[3] = -np.abs(w[3])                                   # class 3: every product <= 0, the map all negative
    w[4] = np.abs(w[4])                                    # class 4: a positive map
    wb = R.f32_to_bf16_bits(w)
    x = R.bf16_bits_to_f32(xb).copy()
    x[:, 1] *= 0.25
    x[:, 1, 40] = x[:, 1, 11] = 4.0                        # frame 1: cells 11 and 40 hold the same values, the largest
    xb = R.f32_to_bf16_bits(x)
    xb[1, 0, 5, 77] = 0x7FC0                               # frame 0: one NaN channel value in cell 5 of sample 1
    classes = [[3, 4, 0, 4], [4, 3, 4, 9]]
    got = run_cam(lib, xb, wb, bias, classes, Hf, Wf)
    check_against_reference(got, xb, wb, bias, classes, Wf)
    r = unpack_cam_records(got[2])
    # frame 1 (no NaN): the all-negative map has a peak and no extent; the equal peaks go to the lower cell
    assert r["peak"][1, 1] < 0 and r["n_above"][1, 1] == 0 and r["box"][1, 1] == -1 and r["pos_sum"][1, 1] == 0
    assert got[1][1, 0, 11] == got[1][1, 0, 40] == r["peak"][1, 0] and r["peak_cell"][1, 0] == 11
    # frame 0: the NaN stays in its cell; the sums carry it, the scans pass over it
    assert np.isnan(got[1][0, :, 5]).all() and np.isnan(got[1][0, :, :5]).sum() == 0 and np.isnan(got[1][0, :, 6:]).sum() == 0
    assert np.isnan(r["logit_mean"][0]).all() and (r["peak_cell"][0] != 5).all() and not np.isnan(r["pos_sum"][0]).any()


@pytest.mark.parametrize("Cc", [2048, 4096])       # 2048 first: the limit is raised once a process
def test_op_cam_the_largest_shapes_in_range(lib, Cc):
    """K = 8 with 1024 cells: C = 4096 fills the 64 KB of weight rows and the 32 KB of maps, above the default LDS limit; at
    C = 2048 the two are exactly 64 KB, and only the kernel's static LDS beside them takes the launch over the limit."""
    S, n, Hf, Wf, K = 1, 2, 4, 256, 8
    xb, wb, bias = problem(9, S, n, Hf * Wf, Cc)
    classes = classes_for(np.random.default_rng(10), n, K)
    got = run_cam(lib, xb, wb, bias, classes, Hf, Wf)
    check_against_reference(got, xb, wb, bias, classes, Wf)
    assert (unpack_cam_records(got[2])["x1"][:, 0] > 127).any()      # a coordinate that needs the whole byte


def test_op_cam_refusals_launch_nothing(lib):
    xb, wb, bias = problem(1, 2, 2, 16, 512, 520)
    classes = [[1, 2], [3, 4]]
    assert run_cam(lib, xb, wb, bias, classes, 4, 4)[0] == 0
    bad = [(dict(S=0), "S=0"), (dict(S=4097), "S=4097"), (dict(n=0), "n must"), (dict(Hf=0), "Hf=0"), (dict(Wf=-1), "Wf=-1"),
           (dict(Hf=33, Wf=32), "cells"), (dict(Hf=1, Wf=257), "sides"), (dict(C=0), "C=0"), (dict(C=256), "C=256"),
           (dict(C=768), "C=768"), (dict(C=4608), "C=4608"), (dict(ldw=504), "ldw=504"), (dict(ldw=516), "ldw=516"),
           (dict(n_classes=0), "n_classes"), (dict(K=0), "K=0"), (dict(K=9), "K=9"),
           (dict(null=("maps",)), "null"), (dict(null=("w",)), "null"), (dict(null=("bias",)), "null"),
           (dict(null=("classes",)), "null"), (dict(null=("cam",)), "null"), (dict(null=("rec",)), "null")]
    for over, text in bad:
        st, _, _, guards, untouched = run_cam(lib, xb, wb, bias, classes, 4, 4, **over)
        msg = lib.fav_last_error(None).decode()
        assert st == 1 and "fav_op_cam" in msg and text in msg, (over, msg)
        assert guards and untouched, over
    # misaligned buffers
    s = torch.cuda.current_stream().cuda_stream
    t = [dev(xb.view(np.int16)), dev(wb.view(np.int16)), dev(bias), dev(np.asarray(classes, np.int32))]
    cam, rec = guarded(2 * 2 * 16 * 4), guarded(2 * 2 * 32)

    def call(maps=0, w=0, cam_off=0, rec_off=0):
        return lib.fav_op_cam(t[0].data_ptr() + maps, 2, 2, 4, 4, 512, t[1].data_ptr() + w, 520, t[2].data_ptr(), NC, t[3].data_ptr(), 2,
                              cam.data_ptr() + GUARD + cam_off, rec.data_ptr() + GUARD + rec_off, s)
    for kw, text in ((dict(maps=8), "16-byte"), (dict(w=2), "16-byte"), (dict(cam_off=2), "4-byte"), (dict(rec_off=4), "8-byte")):
        assert call(**kw) == 1 and text in lib.fav_last_error(None).decode(), kw
    torch.cuda.synchronize()
    assert (cam.cpu().numpy() == FILL).all() and (rec.cpu().numpy() == FILL).all()
    assert call() == 0


# ---- fav_op_cam_heatmap ----------------------------------------------------------------------------------------------------
def run_heatmap(lib, M, rec, hf, wf, h, w, **over):
    m = M.shape[0]
    a = dict(m=m, Hf=hf, Wf=wf, H=h, W=w)
    a.update(over)
    td, rd = dev(np.asarray(M, np.float32)), dev(np.asarray(rec, np.int32))
    out = guarded(m * h * w)
    st = lib.fav_op_cam_heatmap(td.data_ptr(), rd.data_ptr(), a["m"], a["Hf"], a["Wf"], a["H"], a["W"], out.data_ptr() + GUARD,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    body = out.cpu().numpy()[GUARD:GUARD + m * h * w]
    return st, body.reshape(m, h, w).copy(), guards_ok(out, m * h * w), bool((body == FILL).all())


@pytest.mark.parametrize("hw_in,hw_out", [((7, 7), (224, 224)), ((4, 4), (32, 32)), ((8, 10), (240, 320)), ((1, 1), (5, 3))])
def test_op_cam_heatmap_matches_the_reference(lib, hw_in, hw_out):
    (Hf, Wf), (H, W) = hw_in, hw_out
    rng = np.random.default_rng(Hf * 10 + Wf)
    M = rng.standard_normal((5, Hf * Wf)).astype(np.float32)
    M[1] = 0.75                                            # a flat map
    M[2, 0] = np.nan                                       # a NaN cell
    classes = np.array([[0], [0], [0], [0], [7]])          # the last record: a class out of range
    rec = R.cam_records(M[:, None, :], classes, np.zeros(1, np.float32), 1, Wf)[:, 0]
    st, out, guards, _ = run_heatmap(lib, M, rec, Hf, Wf, H, W)
    assert st == 0 and guards
    want = R.heatmap(M, rec, Hf, Wf, H, W)
    assert np.array_equal(out, want)
    assert not out[1].any() and not out[4].any()
    if Hf * Wf > 1:
        assert out[0].any() and out[3].any()


def test_op_cam_heatmap_refusals_launch_nothing(lib):
    M = np.zeros((2, 16), np.float32)
    rec = np.zeros((2, 8), np.int32)
    for over, text in ((dict(m=0), "m must"), (dict(Hf=0), "Hf=0"), (dict(Hf=64, Wf=32), "cells"), (dict(H=0), "H=0"), (dict(W=-3), "W=-3")):
        st, _, guards, untouched = run_heatmap(lib, M, rec, 4, 4, 8, 8, **over)
        msg = lib.fav_last_error(None).decode()
        assert st == 1 and "fav_op_cam_heatmap" in msg and text in msg, (over, msg)
        assert guards and untouched
    assert lib.fav_op_cam_heatmap(None, None, 1, 1, 1, 1, 1, None, None) == 1 and "null" in lib.fav_last_error(None).decode()


# ---- end to end on synthetic checkpoints ---------------------------------------------------------------------------------
def fc_of(blob):
    """-> (w_bits [num_classes, D], bias fp32) of a checkpoint's fc."""
    fc = O.parse_blob(blob).layers[-1]
    return R.f32_to_bf16_bits(fc.w.reshape(fc.cout, -1)), fc.b.astype(np.float32)


def bits_of(t):
    """a bf16 / fp32 CUDA tensor -> its bits on the host."""
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy().view(np.uint16 if t.dtype == torch.bfloat16 else np.uint32)


E2E = {
    "r18_single": dict(arch="resnet18_cifar", hw=(32, 32), n=5, kw=dict(), pooled=False, S=1, chunks=dict(chunk_a=2, chunk_b=3)),
    "r18_mc_all_blocks": dict(arch="resnet18_cifar", hw=(32, 32), n=5, kw=dict(n_samples=3, dropout_policy="all_blocks", dropout_p=0.1, seed=4),
                              pooled=False, S=3, chunks=dict(chunk_a=4, chunk_b=7)),
    "r18_mc_pooled_only": dict(arch="resnet18_cifar", hw=(32, 32), n=5, kw=dict(n_samples=3, dropout_policy="last_layer", dropout_p=0.1, seed=4),
                               pooled=True, S=1, chunks=dict(chunk_a=2, chunk_b=2)),
    "r50_64": dict(arch="resnet50", hw=(64, 64), n=3, kw=dict(), pooled=False, S=1, chunks=dict(chunk_a=1, chunk_b=2)),
    # odd frame sizes: a 2 x 2 map (33 -> 17 -> 9 -> 5 -> 3 -> 2, 47 -> 24 -> 12 -> 6 -> 3 -> 2) upsampled to 33 x 47, and a 4 x 6 one
    "r50_33x47": dict(arch="resnet50", hw=(33, 47), n=3, kw=dict(), pooled=False, S=1, chunks=dict(chunk_a=1, chunk_b=2)),
    "r18_31x45": dict(arch="resnet18_cifar", hw=(31, 45), n=5, kw=dict(n_samples=3, dropout_policy="all_blocks", dropout_p=0.1, seed=4),
                      pooled=False, S=3, chunks=dict(chunk_a=4, chunk_b=7)),
}
# (Hf, Wf) of the map: fav_map_tap_info's, which tests/test_odd_frames_host.py holds to the oracle's shapes at every size
E2E_MAPS = {"r18_single": (4, 4), "r18_mc_all_blocks": (4, 4), "r18_mc_pooled_only": (4, 4), "r50_64": (2, 2), "r50_33x47": (2, 2),
            "r18_31x45": (4, 6)}


@pytest.mark.parametrize("case", list(E2E))
def test_end_to_end(case, r18_blob, r50_blob):
    c = E2E[case]
    blob = (r18_blob if c["arch"] == "resnet18_cifar" else r50_blob)[0]
    n, hw = c["n"], c["hw"]
    frames = torch.from_numpy(synth.synthetic_frames_u8(n, hw[0], hw[1], seed=11)).cuda()
    wb, bias = fc_of(blob)
    NCLS, D = wb.shape
    be = Backend(c["arch"], blob, max_batch=8, in_hw=hw, **c["kw"])
    try:
        info = be.map_tap_info()
        Hf, Wf = info["hf"], info["wf"]
        assert (Hf, Wf) == E2E_MAPS[case]
        assert info == dict(bytes=c["S"] * 8 * Hf * Wf * D * 2, samples=c["S"], hf=Hf, wf=Wf, c=D)
        # 1. the tap changes no result
        off = [t.cpu().numpy() for t in be.classify_detect(frames)] + [bits_of(be.logits())]
        be.set_map_tap(True)
        be.set_feature_tap(True)
        on = [t.cpu().numpy() for t in be.classify_detect(frames)] + [bits_of(be.logits())]
        for a, b in zip(off, on):
            assert np.array_equal(a, b)
        logits = be.logits().cpu().numpy()
        maps = be.maps()
        assert tuple(maps.shape) == (c["S"], n, Hf, Wf, D) and maps.dtype == torch.bfloat16
        xb = bits_of(maps).reshape(c["S"], n, Hf * Wf, D)
        assert np.isfinite(R.bf16_bits_to_f32(xb)).all() and (R.bf16_bits_to_f32(xb) > 0).mean() > 0.05
        # 2. the maps, pooled by the average pool's contract, are the features the fc read
        feats = be.features()
        if not c["pooled"]:
            assert np.array_equal(R.pool(xb), R.f32_to_bf16_bits(feats.cpu().numpy()))
        # 3. classify_cam: fav_classify_ex unchanged, then the head on the predicted class
        out = be.classify_cam(frames, heatmap=True)
        for a, key in zip(on, ("label", "conf", "fail", "score")):
            assert np.array_equal(a, out[key].cpu().numpy()), key
        assert np.array_equal(bits_of(be.maps()).reshape(xb.shape), xb)
        labels = on[0]
        Mr, rr = R.cam(xb, wb, bias, labels[:, None], NCLS, Wf)
        assert R.same_bits(out["map"].cpu().numpy().reshape(n, 1, Hf * Wf), Mr)
        want = unpack_cam_records(rr[:, 0])
        for key, v in want.items():
            assert R.same_bits(out[key].cpu().numpy(), np.ascontiguousarray(v)), key
        assert np.array_equal(out["class_id"].cpu().numpy(), labels)
        assert np.array_equal(out["heatmap"].cpu().numpy(), R.heatmap(Mr[:, 0], rr[:, 0], Hf, Wf, hw[0], hw[1]))
        # 4. cam(top-5) after classify_uncertainty: no second pass, any classes
        unc = be.classify_uncertainty(frames)
        top5 = unc["top_label"]
        assert np.array_equal(top5[:, 0].cpu().numpy(), labels)
        got = be.cam(top5)
        M5, r5 = R.cam(xb, wb, bias, top5.cpu().numpy(), NCLS, Wf)
        assert R.same_bits(got["map"].cpu().numpy().reshape(n, 5, Hf * Wf), M5)
        for key, v in unpack_cam_records(r5).items():
            assert R.same_bits(got[key].cpu().numpy(), np.ascontiguousarray(v)), key
            assert R.same_bits(got[key][:, 0].cpu().numpy(), out[key].cpu().numpy()), key
        assert R.same_bits(got["map"][:, 0].cpu().numpy(), out["map"].cpu().numpy())
        host = be.cam(top5.cpu().numpy()[:, :2])               # numpy in -> numpy out
        assert isinstance(host["map"], np.ndarray) and R.same_bits(host["map"], got["map"][:, :2].cpu().numpy())
        # 5. the decomposition, against the logits the matrix pipe produced
        if not c["pooled"]:
            x64 = R.bf16_bits_to_f32(xb).astype(np.float64)
            w64 = R.bf16_bits_to_f32(wb).astype(np.float64)
            cls = top5.cpu().numpy()
            lm = got["logit_mean"].cpu().numpy().astype(np.float64)
            for i in range(n):
                for k in range(5):
                    cc = cls[i, k]
                    mean_logit = logits[:, i, cc].astype(np.float64).mean()
                    bound = 2.0 ** -8 * (np.abs(w64[cc])[None, :] * x64[:, i].mean(axis=1)).sum(axis=1).mean()
                    assert abs(lm[i, k] - mean_logit) <= bound, (i, k, lm[i, k], mean_logit, bound)
        # 6. chunking: several chunks a phase leave the same maps
        chunked = Backend(c["arch"], blob, max_batch=8, in_hw=hw, **c["kw"], **c["chunks"])
        try:
            chunked.set_map_tap(True)
            lab2, _ = chunked.classify(frames)
            assert np.array_equal(lab2.cpu().numpy(), labels)
            assert np.array_equal(bits_of(chunked.maps()).reshape(xb.shape), xb)
        finally:
            chunked.close()
        # turning the tap off is never refused, and the feature tap does not care
        be.set_map_tap(False)
        assert np.array_equal(bits_of(be.features()), bits_of(feats))
        with pytest.raises(_lib.FavError, match="map tap is off"):
            be.maps()
    finally:
        be.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_handle_refusals(r18_blob):
    blob = r18_blob[0]
    frames = torch.from_numpy(synth.synthetic_frames_u8(4, 32, 32, seed=3)).cuda()
    be = Backend("resnet18_cifar", blob, max_batch=8)
    try:
        cls = torch.zeros((4, 1), dtype=torch.int32, device="cuda")
        be.classify(frames)
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_cam: the map tap is off"):
            be.cam(cls)
        cam = torch.empty((4, 1, 16), dtype=torch.float32, device="cuda")
        rec = torch.empty((4, 1, 8), dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream

        def fav_cam(K=1):
            st = be.lib.fav_cam(be._h, cls.data_ptr(), K, cam.data_ptr(), rec.data_ptr(), s)
            return st, be.lib.fav_last_error(be._h).decode()
        st, msg = fav_cam()
        assert st == 1 and "fav_cam: the map tap is off" in msg
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_classify_cam: the map tap is off"):
            be.classify_cam(frames)
        # over the budget: both numbers
        need = 8 * 16 * 512 * 2
        with pytest.raises(_lib.FavError, match=f"FAV_ERR_INVALID_ARG.*fav_set_map_tap.*{need} bytes.*max_bytes={need - 1}"):
            be.set_map_tap(True, budget_bytes=need - 1)
        be.set_map_tap(True, budget_bytes=need)
        st, msg = fav_cam()
        assert st == 1 and "fav_cam: no classify call since the tap was turned on" in msg
        with pytest.raises(_lib.FavError, match="fav_get_maps: no classify call"):
            be.maps()
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_cam: no classify call"):
            be.cam(cls)
        be.classify(frames)
        assert fav_cam()[0] == 0
        plain = bits_of(be.maps())
        st, msg = fav_cam(K=9)
        assert st == 1 and "fav_cam: K=9" in msg
        # views: the maps are there, the head is not
        be.set_views(views.hflip())                             # the frame and its mirror image
        st, msg = fav_cam()
        assert st == 6 and "fav_cam: views are set" in msg
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_classify_cam: views are set"):
            be.classify_cam(frames)
        be.classify(frames)
        m = be.maps()
        assert tuple(m.shape) == (2, 4, 4, 4, 512)
        assert np.array_equal(bits_of(m[0]), plain[0])                   # sample a is view a: the identity's maps first
        assert not np.array_equal(bits_of(m[1]), plain[0])
        be.set_views(None)
        st, msg = fav_cam()
        assert st == 6 and "fav_cam: the last call ran under views" in msg
        be.classify(frames)
        assert fav_cam()[0] == 0
        be.set_map_tap(False)
        be.set_map_tap(False)
    finally:
        be.close()


def test_map_tap_refused_on_vit_and_on_an_ensemble(r18_blob):
    vblob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
    vit = Backend("vit_tiny", vblob, max_batch=4)
    try:
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_set_map_tap.*ViT"):
            vit.set_map_tap(True)
        vit.set_map_tap(False)                                  # turning it off is never refused
    finally:
        vit.close()
    ens = Backend("resnet18_cifar", [r18_blob[0], r18_blob[0]], max_batch=4)
    try:
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_set_map_tap.*ensemble"):
            ens.set_map_tap(True)
        ens.set_map_tap(False)
    finally:
        ens.close()
