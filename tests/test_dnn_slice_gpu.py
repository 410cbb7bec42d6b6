"""CNN / SGAN classification of target slices on the GPU: rml_dnn_preprocess_slices (csrc/preprocess_slice.hip: the three planes through
a target's voxel, from the volume into the preprocessing kernel's LDS image, T targets per frame, one launch) and what is wired on top
of it -- Classifier.predict_volumes / Discriminator.predict_volumes with mode="slice", ijk=(B,T,3) or derived targets, the margin
guard's re-scoring of slice rows, predict.classify_targets.  The reference of every check is NumPy slicing of the host volume
(predict.py:98-107) through the Pillow-exact resize (tests/dnn_slice_common.py)."""
import functools
import gc
import importlib

import numpy as np
import pytest
import torch

import dnn_slice_common as S

pytestmark = pytest.mark.gpu

RML_OK, RML_ERR_INVALID, RML_ERR_UNSUPPORTED = 0, -1, -2
# tests/test_nn_gpu.py:407, applied to predict_volumes (mode "max") against the float64 restatement of the layers at :176
DNN_BF16_PROBA_TOL = 8e-3
# tests/test_sgan_infer_gpu.py:17, applied to Discriminator.predict_volumes against its plain float32 layers at :204 (2 x E_p + this)
PREPROCESS_ALLOWANCE = 2e-4
WALABOT = (22, 31, 176)


@pytest.fixture(scope="module")
def nc(rml):
    return importlib.import_module("radar_ml_amd.nn_common")


@pytest.fixture(autouse=True)
def _global_rng_untouched():
    """the tests that run after this file see the global random streams they would see without it (some draw dropout masks from them)"""
    with torch.random.fork_rng(devices=[torch.cuda.current_device()]):
        yield


@pytest.fixture(scope="module")
def disc(rml):
    """(the 128 x 128 test Discriminator of tests/sgan_infer_common.py, its yardstick E_p).  The shared caches are emptied again, so
    that tests/test_sgan_infer_gpu.py builds its cases where it always did."""
    from sgan_infer_common import case, yardstick
    with torch.random.fork_rng(devices=[torch.cuda.current_device()]):
        _, e_p = yardstick()
        model = case(128, 128, 9, 3, 5)[0]
    yield model, e_p
    case.cache_clear()
    yardstick.cache_clear()


@functools.lru_cache(maxsize=None)
def _case(grid, rescale, kind):
    """(host volumes, CUDA volumes, (B,3,3) targets, exact bf16 planes, exact float32 planes) of one case: computed once, shared"""
    nc_ = importlib.import_module("radar_ml_amd.nn_common")
    vol, ijk = S.volumes(grid, kind), S.targets(grid)
    return (vol, torch.from_numpy(vol).cuda(), ijk, S.exact_planes(nc_, vol, ijk, rescale, "bfloat16"),
            S.exact_planes(nc_, vol, ijk, rescale, "float32"))


def _slices(nc, v, ijk, rescale):
    """rml_dnn_preprocess_slices on (B,T,3) host targets"""
    from radar_ml_amd import common
    B, X, Y, Z = (int(t) for t in v.shape)
    ijk_t, T = common._slice_indices(ijk, B, X, Y, Z, v.device)
    return nc.preprocess_slices(v, ijk_t, T, rescale)


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("grid,rescale", S.GRIDS)
def test_planes(rml, nc, grid, rescale, kind):
    """T = 3 and T = 1 (every column of the targets) on B = 3 frames.  (a) within one bf16 ulp of the Pillow-exact planes of the
    NumPy slices and 2^-8 of their float32 values; (b) bit-identical to preprocess_rows on the rows of process_volumes(mode="slice",
    ijk=(B,T,3)) with the kernel's staging type -- code rows for uint8 volumes (float16 images), float rows for float32 volumes;
    (c) row b*T+t of the (B,T,3) call is the row of the (B,3) call with ijk[:, t], bit for bit -- through the entry point and
    through nn_common.preprocess_volumes, whose (B,3) call keeps the code-row route."""
    assert nc.preprocess_supported(grid, rescale)
    vol, v, ijk, want16, want32 = _case(grid, rescale, kind)
    got = _slices(nc, v, ijk, rescale)
    S.check_against_exact(got, want16, want32, "slices %s -> %s %s T=3" % (grid, rescale, kind))                   # (a)
    if kind == "u8":                                                                                                # (b)
        codes = rml.process_volumes(v, mode="slice", ijk=ijk, scale=False, codes="only")[1]
        rows = nc.preprocess_rows(grid, rescale, codes=codes)
    else:
        rows = nc.preprocess_rows(grid, rescale, feat=rml.process_volumes(v, mode="slice", ijk=ijk, scale=False))
    front = nc.preprocess_volumes(v, rescale, mode="slice", ijk=ijk)
    for pl in range(3):
        assert torch.equal(got[pl], rows[pl]), (pl, "preprocess_rows on the sliced rows")
        assert torch.equal(got[pl], front[pl]), (pl, "preprocess_volumes (B,T,3)")
    for t in range(3):                                                                                              # (c), and T = 1
        one = _slices(nc, v, ijk[:, t:t + 1], rescale)
        S.check_against_exact(one, [w[t::3] for w in want16], [w[t::3] for w in want32], "slices %s %s T=1 column %d" % (grid, kind, t))
        per_frame = nc.preprocess_volumes(v, rescale, mode="slice", ijk=ijk[:, t])
        for pl in range(3):
            assert torch.equal(got[pl][t::3], one[pl]), (pl, t)
            assert torch.equal(got[pl][t::3], per_frame[pl]), (pl, t, "the (B,3) route")


def test_uint8_and_float32_volumes_of_the_same_integers_give_the_same_bits(rml, nc):
    for grid, rescale in S.GRIDS:
        a = _slices(nc, _case(grid, rescale, "u8")[1], S.targets(grid), rescale)
        b = _slices(nc, _case(grid, rescale, "f32_grid")[1], S.targets(grid), rescale)
        for pl in range(3):
            assert torch.equal(a[pl], b[pl])


def test_derived_targets_and_return_ijk(rml, nc):
    grid, rescale = S.GRIDS[1]
    v = _case(grid, rescale, "u8")[1]
    want = rml.derive_targets(v, 2)
    got, used = nc.preprocess_volumes(v, rescale, mode="slice", ijk=None, num_targets=2, return_ijk=True)
    assert used.dtype == torch.int32 and used.shape == (S.B, 2, 3) and torch.equal(used, want)
    given = nc.preprocess_volumes(v, rescale, mode="slice", ijk=want)
    for pl in range(3):
        assert got[pl].shape[0] == 2 * S.B and torch.equal(got[pl], given[pl])


def test_last_frame_beyond_2_31_voxels(rml, nc):
    """(d) a uint8 batch whose last frame starts beyond 2^31 voxels (2.15 GB) at the smallest rescale the kernel takes for the grid:
    the first and the last 8 rows against (a)."""
    grid = WALABOT
    X, Y, Z = grid
    per = X * Y * Z
    B = (1 << 31) // per + 2
    assert (B - 1) * per > 1 << 31
    gc.collect(); torch.cuda.empty_cache()              # what earlier tests left in the allocator's cache counts as used
    if torch.cuda.mem_get_info()[0] < B * per + (1 << 30):
        pytest.skip("needs %.1f GB of free device memory" % ((B * per + (1 << 30)) / 1e9))
    oh = 32
    rescale = next((ow, oh) for ow in range(4, 260, 4) if nc.preprocess_supported(grid, (ow, oh)))
    g = torch.Generator(device="cuda").manual_seed(5)
    v = torch.randint(0, 256, (B, X, Y, Z), dtype=torch.uint8, device="cuda", generator=g)
    rng = np.random.default_rng(6)
    ijk = np.stack([rng.integers(-X, X, B), rng.integers(-Y, Y, B), rng.integers(-Z, Z, B)], axis=1).astype(np.int32)[:, None, :]
    ijk[-1, 0] = (X - 1, Y - 1, Z - 1)                  # the last voxel of the batch is read
    got = _slices(nc, v, ijk, rescale)
    torch.cuda.synchronize()
    for sl in (slice(0, 8), slice(B - 8, B)):
        host = v[sl].cpu().numpy()
        want16 = S.exact_planes(nc, host, ijk[sl], rescale, "bfloat16")
        want32 = S.exact_planes(nc, host, ijk[sl], rescale, "float32")
        S.check_against_exact([p[sl] for p in got], want16, want32, "rows %s of %d at %s" % (sl, B, rescale))
    del v, got
    gc.collect(); torch.cuda.empty_cache()


def test_c_abi_argument_checks(rml):
    from radar_ml_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    ctx, st = _lib.context(dev), _lib.stream_ptr(dev)
    X, Y, Z = 5, 7, 16
    v = torch.zeros((2, X, Y, Z), dtype=torch.uint8, device="cuda")
    ijk = torch.zeros((2, 2, 3), dtype=torch.int32, device="cuda")
    outs = [torch.full((4, 16, 16), 7.0, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    p = _lib.ptr

    def call(vol=v, vdt=_lib.VOL_U8, B=2, grid=(X, Y, Z), idx=ijk, T=2, hw=(16, 16), o=outs, c=ctx):
        return lib.rml_dnn_preprocess_slices(c, p(vol), vdt, B, grid[0], grid[1], grid[2], p(idx), T, hw[0], hw[1], p(o[0]), p(o[1]), p(o[2]), st)
    assert call() == RML_OK
    for k in range(3):
        assert call(o=[None if j == k else outs[j] for j in range(3)]) == RML_ERR_INVALID          # NULL outputs
    assert call(vol=None) == RML_ERR_INVALID and call(idx=None) == RML_ERR_INVALID and call(c=None) == RML_ERR_INVALID
    assert call(T=0) == RML_ERR_INVALID and call(T=-1) == RML_ERR_INVALID
    assert call(B=-1) == RML_ERR_INVALID and call(vdt=7) == RML_ERR_INVALID
    assert call(grid=(X, Y, 20)) == RML_ERR_UNSUPPORTED                                             # Z % 16
    assert call(hw=(2, 16)) == RML_ERR_UNSUPPORTED                                                  # the height shrinks 3.5 x: 7-tap windows
    assert call(hw=(16, 18)) == RML_ERR_UNSUPPORTED                                                 # out_w % 4
    assert call(B=0) == RML_OK and call(B=0, vol=None, idx=None, o=[None] * 3) == RML_OK
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).sum() == 0) for o in outs)                                           # the good call wrote every row


# ---- end to end: Classifier -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _classifier():
    dnn = importlib.import_module("radar_ml_amd.dnn")
    torch.manual_seed(11)
    return dnn.define_classifier(device="cuda").eval()


@functools.lru_cache(maxsize=None)
def _frames(n=16):
    import oracle_np as O
    vol, _ = O.synth_volumes(41, n, *WALABOT)
    return vol.astype(np.float32)


def _float64(nc, model, vol, ijk, rescale=(80, 80)):
    """the float64 restatement of the layers on the NumPy-sliced, Pillow-exact planes: (B*T, C) float64"""
    ijk = np.asarray(ijk)
    with torch.no_grad():
        return model.forward_exact(*S.exact_planes(nc, vol, ijk.reshape(len(vol), -1, 3), rescale, "float32"), precision="float64")


def test_classifier_labels_and_probabilities_against_float64(rml, nc):
    model = _classifier()
    vol, ijk = _frames()[:S.B], S.targets(WALABOT)
    want = _float64(nc, model, vol, ijk)
    for v in (torch.from_numpy(vol).cuda(), torch.from_numpy(vol.astype(np.uint8)).cuda(), torch.from_numpy(vol)):
        got = model.predict_volumes(v, mode="slice", ijk=ijk)
        assert got.shape == (9, 3) and got.dtype == torch.float32 and got.is_cuda
        err = float((got.double() - want).abs().max())
        print("predict_volumes(slice, (3,3,3)) against float64: max |dp| = %.3e, guard re-scored %d rows" % (err, model.last_guard["rescored"]))
        assert torch.equal(got.argmax(1), want.argmax(1))
        assert err <= DNN_BF16_PROBA_TOL
    # the route of the grids and rescales the fused kernel does not take, and of exact_resize=True: the same (B,T,3) semantics
    exact = model.predict_volumes(torch.from_numpy(vol).cuda(), mode="slice", ijk=ijk, exact_resize=True)
    assert torch.equal(exact.argmax(1), want.argmax(1)) and float((exact.double() - want).abs().max()) <= DNN_BF16_PROBA_TOL
    # mode "max" ignores the new arguments
    v = torch.from_numpy(vol).cuda()
    assert torch.equal(model.predict_volumes(v, label_guard=None), model.predict_volumes(v, label_guard=None, ijk=ijk, num_targets=2))


def test_classifier_per_target_calls_and_derived_targets(rml, nc):
    model = _classifier()
    v = torch.from_numpy(_frames()[:S.B]).cuda()
    ijk = S.targets(WALABOT)
    whole = model.predict_volumes(v, mode="slice", ijk=ijk, label_guard=None)
    for t in range(3):
        one = model.predict_volumes(v, mode="slice", ijk=ijk[:, t], label_guard=None)
        assert one.shape == (S.B, 3) and torch.equal(whole[t::3], one)
    assert torch.equal(model.predict_volumes(v, mode="slice", ijk=ijk, label_guard=None, batch_size=2), whole)      # two passes
    derived = rml.derive_targets(v, 2)
    got, used = model.predict_volumes(v, mode="slice", ijk=None, num_targets=2, return_ijk=True, label_guard=None)
    assert used.dtype == torch.int32 and torch.equal(used, derived) and got.shape == (2 * S.B, 3)
    assert torch.equal(got, model.predict_volumes(v, mode="slice", ijk=derived, label_guard=None))
    guarded, used = model.predict_volumes(v, mode="slice", num_targets=2, return_ijk=True)
    assert torch.equal(used, derived) and torch.equal(guarded.argmax(1), _float64(nc, model, _frames()[:S.B], derived.cpu().numpy()).argmax(1))


def test_guard_rescores_a_slice_row_inside_the_gap(rml, nc):
    """One target is built to sit inside the guard gap: the average (weights found by bisection) of two frames whose float64 labels
    at that voxel differ.  The guard re-scores it -- row r from frame r // T at ijk[r] -- and every row lands on the float64 label."""
    dnn = importlib.import_module("radar_ml_amd.dnn")
    model = _classifier()
    frames = _frames()
    at = np.array([11, 15, 88], dtype=np.int32)
    lab = _float64(nc, model, frames, np.tile(at, (len(frames), 1))).argmax(1).cpu().numpy()
    assert len(set(lab.tolist())) > 1, "every frame has the same float64 label at %s: no pair to average" % (at,)
    a = 0
    b = int(np.nonzero(lab != lab[a])[0][0])
    lo, hi = 0.0, 1.0                   # weight of frame b: label(lo) == lab[a], label(hi) != lab[a]
    gap = 1.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        blend = ((1.0 - mid) * frames[a] + mid * frames[b]).astype(np.float32)
        p = _float64(nc, model, blend[None], at[None])[0]
        top = torch.sort(p, descending=True).values
        gap = float(top[0] - top[1])
        if gap < dnn.LABEL_GUARD / 10:
            break
        if int(p.argmax()) == lab[a]:
            lo = mid
        else:
            hi = mid
    assert gap < dnn.LABEL_GUARD / 10
    vol = np.stack([frames[2], blend, frames[3]])
    ijk = S.targets(WALABOT).copy()
    ijk[1, 1] = at
    want = _float64(nc, model, vol, ijk)
    got = model.predict_volumes(torch.from_numpy(vol).cuda(), mode="slice", ijk=ijk)
    print("guard on slices: %s; float64 gap of the built row %.2e" % (model.last_guard, gap))
    assert model.last_guard["rescored"] >= 1
    assert torch.equal(got.argmax(1), want.argmax(1))
    assert float((got.double() - want).abs().max()) <= DNN_BF16_PROBA_TOL
    # rescore_exact by itself: unsorted rows with a repeat map to (frame, target) = (r // 3, r % 3)
    rows = torch.tensor([7, 4, 0, 4], device="cuda")
    again = model.rescore_exact(torch.from_numpy(vol).cuda(), mode="slice", precision="float64", rows=rows, ijk=ijk)
    assert float((again - want[rows]).abs().max()) <= 1e-12
    everything = model.rescore_exact(torch.from_numpy(vol), mode="slice", precision="float64", ijk=ijk)         # host volumes, all rows
    assert float((everything - want).abs().max()) <= 1e-12


# ---- end to end: Discriminator, classify_targets -----------------------------------------------------------------------------

def test_discriminator_targets(rml, nc, disc):
    from sgan_infer_common import plain_eval, check_labels
    model, e_p = disc
    vol, ijk = _frames()[:S.B], S.targets(WALABOT)
    v = torch.from_numpy(vol).cuda()
    assert nc.preprocess_supported(WALABOT, (128, 128))
    p_ref = plain_eval(model, S.exact_planes(nc, vol, ijk, (128, 128), "float32"))[1]
    whole = model.predict_volumes(v, mode="slice", ijk=ijk, return_numpy=False)
    err = float((whole - p_ref).abs().max())
    print("Discriminator.predict_volumes(slice, (3,3,3)): |dp| = %.3e (2 x E_p = %.3e)" % (err, 2 * e_p))
    assert whole.shape == (9, 3) and err <= 2 * e_p + PREPROCESS_ALLOWANCE
    check_labels(whole, p_ref, e_p, "Discriminator slices")
    exact = model.predict_volumes(v, mode="slice", ijk=ijk, exact_resize=True, return_numpy=False)
    assert float((exact - p_ref).abs().max()) <= 2 * e_p
    for t in range(3):
        assert torch.equal(whole[t::3], model.predict_volumes(v, mode="slice", ijk=ijk[:, t], return_numpy=False))
    assert torch.equal(model.predict_volumes(v.to(torch.uint8), mode="slice", ijk=ijk, batch_size=2, return_numpy=False), whole)
    derived = rml.derive_targets(v, 2)
    got, used = model.predict_volumes(vol, mode="slice", num_targets=2, return_ijk=True)            # host in, numpy out
    assert isinstance(got, np.ndarray) and got.shape == (2 * S.B, 3) and np.array_equal(used, derived.cpu().numpy())
    assert np.array_equal(got, model.predict_volumes(v, mode="slice", ijk=derived))


def test_classify_targets(rml, nc, disc):
    """a hand-made case: the probabilities of predict_volumes decide the names -- 'Unknown' below min_proba, the class name at or
    above it"""
    from radar_ml_amd import predict
    classes = ["cat", "dog", "person"]
    v = torch.from_numpy(_frames()[:S.B]).cuda()
    ijk = S.targets(WALABOT)
    sgan_model = disc[0]                                # no guard: the same call gives the same bits
    p = sgan_model.predict_volumes(v, mode="slice", ijk=ijk)
    top = p.max(1)
    cut = float(np.sort(top)[4])                        # the fifth smallest: rows below it are unknown, rows at or above it named
    names, proba = predict.classify_targets(sgan_model, classes, v, ijk=ijk, min_proba=cut)
    assert len(names) == 9 and np.array_equal(proba, top)
    for r in range(9):
        assert names[r] == (classes[int(p[r].argmax())] if top[r] >= cut else "Unknown")
    assert "Unknown" in names and any(n != "Unknown" for n in names)
    model = _classifier()                               # derived targets, the guard on
    names, proba = predict.classify_targets(model, classes, v, num_targets=2, min_proba=1.1)
    assert names == ["Unknown"] * 6 and proba.shape == (6,)
    names, _ = predict.classify_targets(model, classes, v, num_targets=2, min_proba=0.0)
    assert len(names) == 6 and all(n in classes for n in names)
