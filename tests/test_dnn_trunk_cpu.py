"""Host-side half of the CNN trunk sweep: rml_dnn_trunk_path (the dispatch of csrc/dnn.hip, answered by the launchers' own
predicates) and the cases of tests/dnn_trunk_common.py -- which paths the plane shapes reach, and the conditions the exact-integer
operands must meet for "bit for bit" to mean what tests/test_dnn_trunk_gpu.py takes it to mean.  No GPU; run with -s for the table."""
import copy
import ctypes

import pytest
import torch

import dnn_trunk_common as T

NUM_CU = 256         # the MI355X; the thresholds are checked at other counts too


def test_query_agrees_with_kblock_supported(rml):
    """rml_dnn_trunk_kblock_supported is "the rf kernel takes the plane" for bf16-capable planes with an even pixel count"""
    from radar_ml_amd import _lib
    lib = _lib.load()
    n = 0
    for H in range(4, 204, 4):
        for W in range(8, 264, 8):
            if ((H // 4) * (W // 4)) % 2:
                continue
            rf = T.path(H, W, True).kernel == 1
            assert bool(lib.rml_dnn_trunk_kblock_supported(H, W)) == rf == (T.path(H, W, False).kernel == 1), (H, W)
            n += rf
    assert 100 < n < 50 * 32 // 2
    assert T.path(80, 80, True).kernel == 1 and T.path(88, 80, True).kernel == 1 and T.path(96, 80, True).kernel == 2


def test_query_arguments(rml):
    from radar_ml_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 6)(*([9] * 6))
    p = ctypes.cast(out, ctypes.c_void_p)
    assert lib.rml_dnn_trunk_path(80, 80, 0, 1, 256, None) == -1
    assert lib.rml_dnn_trunk_path(80, 80, 0, 0, 256, p) == -1 and lib.rml_dnn_trunk_path(80, 80, 0, 1 << 31, 256, p) == -1
    assert lib.rml_dnn_trunk_path(80, 80, 0, 1, 0, p) == -1
    assert list(out) == [9] * 6                                        # untouched on an error
    # what rml_dnn_trunk refuses as a shape is "unsupported", not an error: H % 4, W % 4 (W % 8 for bf16 planes), no kernel
    for (H, W, bf) in ((6, 8, 0), (8, 6, 0), (8, 12, 1), (0, 8, 0), (8, -8, 0), T.UNSUPPORTED + (0,), T.UNSUPPORTED + (1,)):
        assert lib.rml_dnn_trunk_path(H, W, bf, 5, 256, p) == 0 and list(out) == [0] * 6, (H, W, bf)
    assert T.path(8, 12, False).kernel == 1


def test_batch_thresholds_come_from_the_query(rml):
    """the batch sizes of the sweep sit where the launchers change behaviour, on any CU count"""
    for num_cu in (1, 2, 3, 80, 256, 304):
        b = T.batches(80, 80, True, num_cu, big=True)
        assert T.path(80, 80, True, 2 * num_cu, num_cu).split == 1 and T.path(80, 80, True, 2 * num_cu + 1, num_cu).split == 0
        assert T.path(80, 80, True, b[-1], num_cu).gx == num_cu and 8 * num_cu < b[-1]          # a wave per sample: some take two
        for (H, W) in ((124, 64), (128, 128), (28, 248)):
            one, two, over, twice = T.batches(H, W, True, num_cu)
            gx = over - 1
            wpc = T.path(H, W, True, 1, num_cu).wpc
            assert gx == max(1, wpc * num_cu // 3)
            assert [T.path(H, W, True, n, num_cu).gx for n in (one, two, over, twice)] == [min(1, gx), min(2, gx), gx, gx]
            assert twice > 2 * gx


def test_shapes_reach_every_reachable_path(rml):
    """SHAPES reaches every (kernel, SR, prefetch, input dtype) that ANY plane up to 512 x 512 reaches; prints the table"""
    reach = {}
    for H in range(4, 516, 4):
        for W in range(4, 516, 4):
            for bf in ((False, True) if W % 8 == 0 else (False,)):
                p = T.path(H, W, bf, 1, NUM_CU)
                if p.kernel:
                    reach.setdefault(T.combo(p) + (bf,), (H, W))
    got = {}
    print("\nplane      planes  kernel          SR WPC prefetch  batches")
    for (H, W, bf) in T.cases():
        p = T.path(H, W, bf, 1, NUM_CU)
        assert p.kernel in (1, 2), (H, W, bf)
        got.setdefault(T.combo(p) + (bf,), (H, W))
        print("%-10s %-7s %-15s %2d %3d %8d  %s" % ("%dx%d" % (H, W), "bf16" if bf else "float32", T.KERNEL_NAMES[p.kernel], p.sr, p.wpc, p.prefetch,
                                                     T.batches(H, W, bf, NUM_CU, big=(H, W) in ((24, 16), (8, 8)))))
    print("%-10s %-7s %s" % ("%dx%d" % T.UNSUPPORTED, "both", T.KERNEL_NAMES[T.path(*T.UNSUPPORTED, False).kernel]))
    assert set(got) == set(reach), (sorted(set(reach) - set(got)), sorted(set(got) - set(reach)))
    # 13 combinations: rf x 2 dtypes; the LDS kernel at SR 4 / 2 / 1 x prefetch on / off x 2 dtypes, less float32 prefetch at SR=2 --
    # a float32 plane prefetches up to 1792 quads (H * W <= 7168), and every such plane that the rf kernel leaves ((H + 4)(W + 4) > 7926)
    # and SR=4 at two workgroups per CU does not take is too wide for SR=2's five pixel tiles (W <= 160); at SR=4 the corner exists
    # (196 x 36 and its like), at SR=1 plenty
    assert len(reach) == 13 and (2, 2, 1, False) not in reach and (2, 4, 1, False) in reach
    # the strips: a partial last strip of every length at SR=4, the one-row one at SR=2, and whole strips
    left = {(T.path(H, W, False).sr, (H // 4) % T.path(H, W, False).sr) for (H, W, _, _) in T.SHAPES if T.path(H, W, False).kernel == 2}
    assert {(4, 0), (4, 1), (4, 2), (4, 3), (2, 0), (2, 1), (1, 0)} <= left
    assert T.path(160, 80, False).sr == 2 and T.path(160, 80, True).sr == 2          # SR=4 fits one workgroup per CU but not two
    assert T.path(*T.UNSUPPORTED, False).kernel == 0 and T.path(*T.UNSUPPORTED, True).kernel == 0
    # real-valued cases: one shape per combination
    assert {T.combo(T.path(H, W, bf)) + (bf,) for (H, W, bf) in T.real_shapes()} == set(reach)


def test_round_bf16_is_nearest_even():
    """the twin's float64 -> bf16 rounding against torch's float32 -> bf16 on float32 values, and at exact ties in both directions"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(20000, generator=g) * torch.tensor(2.0) ** torch.randint(-12, 12, (20000,), generator=g)
    assert torch.equal(T.round_bf16(x.double()), x.to(torch.bfloat16).double())
    assert T.round_bf16(torch.tensor([257.0, 259.0, 511.0, 1.00390625, 1.01171875, -257.0], dtype=torch.float64)).tolist() == \
        [256.0, 260.0, 512.0, 1.0, 1.015625, -256.0]
    # a float64 just above a tie must round up although float32 would first round it ONTO the tie (and then to even, down)
    assert T.round_bf16(torch.tensor([257.0 + 2.0 ** -40], dtype=torch.float64)).item() == 258.0
    y = torch.tensor([0.75, 3.0, 256.0, 300.0, 511.9], dtype=torch.float64)
    assert T.half_ulp_bf16(y).tolist() == [2.0 ** -9, 2.0 ** -7, 1.0, 1.0, 1.0]


def test_twin_is_the_models_layers(rml):
    """on integer operands nothing rounds, so the twin must equal the project's own float64 layers (Classifier.features: the
    TensorFlow 'same' pad of nn_common, Keras' Flatten order) exactly; to_kblock against the layout's index formula"""
    for (H, W) in ((4, 4), (24, 16), (44, 36), (28, 248)):
        m, x = T.int_model(H, W), T.int_planes(H, W)
        y, bits = T.int_twin(H, W)
        with torch.no_grad():
            want = copy.deepcopy(m).double().features(*[p.double()[:, None] for p in x])
        assert y.shape == want.shape == (T.DISTINCT, (H // 4) * (W // 4) * 96) and torch.equal(y, want)
        assert torch.equal(T.twin(m, x, True)[0], y)                      # integer biases: exact as one bf16 too
    H, W = 24, 16
    y, _ = T.int_twin(H, W)
    kb = T.to_kblock(y, H, W)
    P = (H // 4) * (W // 4)
    assert kb.shape == (P * 96 // 64, T.DISTINCT, 64)
    for b in (0, 6):
        for br in range(3):
            for pix in (0, 1, 7, P - 1):
                for ch in (0, 13, 31):
                    assert kb[(br * P + pix) // 2, b, (pix & 1) * 32 + ch] == y[b, pix * 96 + br * 32 + ch]


def test_integer_cases_meet_their_conditions(rml):
    """What makes "equal bit for bit" a theorem: conv1 values are integers of magnitude <= 256 (exact in bf16), conv2 sums stay below
    2^24 (exact in float32 in any order; bounded through sum |w2| * max conv1), the weights and biases are bf16-exact integers.  And what
    makes it a test: outputs on both sides of the relu, outputs above 256 where bf16 cannot hold every integer, exact ties that
    round-to-nearest-even takes down AND up, non-zero plane edges."""
    up = down = 0
    for (H, W, _, _) in T.SHAPES:
        m, x = T.int_model(H, W), T.int_planes(H, W)
        for p in x:
            assert p.shape == (T.DISTINCT, H, W) and torch.equal(p, p.round()) and p.abs().max() <= 3
            assert (p[:, 0] != 0).all() and (p[:, -1] != 0).all() and (p[:, :, 0] != 0).all() and (p[:, :, -1] != 0).all()
        for br in m.branches:
            for t in (br[0].conv.weight, br[0].conv.bias, br[1].conv.weight, br[1].conv.bias):
                assert torch.equal(t, t.round()) and torch.equal(t.to(torch.bfloat16).float(), t.detach())
        c1 = T.conv1_image(m, x, False)
        c1max = max(float(c.abs().max()) for c in c1)
        assert all(torch.equal(c, c.round()) for c in c1) and c1max <= 256
        for c, br in zip(c1, m.branches):
            w2, b2 = br[1].conv.weight.detach().double(), br[1].conv.bias.detach().double()
            assert float(w2.abs().sum(dim=(1, 2, 3)).max()) * c1max + float(b2.abs().max()) < 2 ** 24
        y, bits = T.int_twin(H, W)
        assert torch.equal(y, y.round()) and y.min() == 0
        assert (y > 0).double().mean() >= 0.30, (H, W)
        if (H // 4) * (W // 4) >= 16:                # a conv2 window of a tinier plane holds too few live taps to get there
            assert (y > 256).any(), (H, W)
        r = T.round_bf16(y)
        tie = (y > 256) & (y < 512) & (y % 2 == 1)
        assert torch.equal(bits.view(torch.bfloat16).double(), r) and (r[tie] % 4 == 0).all()
        up += int((tie & (r > y)).sum())
        down += int((tie & (r < y)).sum())
    print("integer cases: %d ties rounded up, %d down" % (up, down))
    assert up >= 1 and down >= 1


def test_fractional_bias_cases_meet_their_conditions(rml):
    """frac_model: conv1 biases of more bits than one bf16 holds, which two (so also the rf kernel's three) bf16 pieces and float32
    hold exactly; every conv1 value and conv2 partial sum a multiple of 2^-8 below 2^16, i.e. exact in float32 in any order -- bit for
    bit again, and the twin's answer depends on whether the bias was carried whole (rf, x3) or as one bf16 (the LDS kernel)"""
    bf = lambda t: t.to(torch.bfloat16).float()
    for (H, W, _, _) in T.SHAPES:
        m, mi, x = T.frac_model(H, W), T.int_model(H, W), T.int_planes(H, W)
        c1max = 0.0
        for br, bri in zip(m.branches, mi.branches):
            b1 = br[0].conv.bias.detach()
            assert torch.equal(b1 * 256, (b1 * 256).round()) and b1.abs().max() < 4 and (bf(b1) != b1).sum() >= 16
            assert torch.equal(bf(b1) + bf(b1 - bf(b1)), b1)                          # two bf16 pieces carry it
            for t, ti in ((br[0].conv.weight, bri[0].conv.weight), (br[1].conv.weight, bri[1].conv.weight), (br[1].conv.bias, bri[1].conv.bias)):
                assert torch.equal(t, ti)
        for flag in (False, True):
            c1 = T.conv1_image(m, x, flag)
            c1max = max(float(c.abs().max()) for c in c1)
            assert all(torch.equal(c * 256, (c * 256).round()) for c in c1) and c1max <= 256
            for br in m.branches:
                w2, b2 = br[1].conv.weight.detach().double(), br[1].conv.bias.detach().double()
                assert float(w2.abs().sum(dim=(1, 2, 3)).max()) * c1max + float(b2.abs().max()) < 2 ** 16
        y, _ = T.int_twin(H, W, True, False)
        yb, _ = T.int_twin(H, W, True, True)
        assert torch.equal(y * 256, (y * 256).round()) and (y > 0).double().mean() >= 0.30
        assert not torch.equal(T.round_bf16(y), T.round_bf16(yb)), (H, W)               # one bf16 of bias: other output BITS
        yx, _ = T.int_twin(H, W, True, False, False)                                   # csrc/dnn_x3.hip: no bf16 conv1 image
        assert torch.equal(yx * 256, (yx * 256).round()) and torch.equal(yx.float().double(), yx) and not torch.equal(yx, y)


def test_real_cases_have_nonzero_edges_and_an_e32(rml):
    """the float32 twin differs from the float64 twin (else E32 would measure nothing)"""
    H, W = 24, 16
    for p in T.real_planes(H, W):
        assert p.abs().max() <= 1 and (p[:, 0] != 0).all() and (p[:, -1] != 0).all() and (p[:, :, 0] != 0).all() and (p[:, :, -1] != 0).all()
    y64, y32 = T.real_twins(H, W, False)
    e32 = float((y64 - y32).abs().max())
    print("real case %dx%d: E32 = %.3e, max output %.3f" % (H, W, e32, float(y64.max())))
    assert e32 > 0
    assert not torch.equal(T.real_twins(H, W, True)[0], y64)           # the bias flag matters on real biases
