"""The training kernels one variant at a time: a single layer L between two helper layers (tests/helpers.py: Probe - dense input ->
a (-> a2) -> L -> fin -> head, L without ReLU so that nothing compared depends on a ReLU mask) through the training entry points,
against float64 autograd, with fp32 ATen autograd on the CPU as the yardstick of what fp32 rounding alone does.

Per case: the activations of a / a2 / L, dW and dgamma / dbeta (or dbias) of L, the gradient tensors of every source of L, the loss.
Two criteria per tensor X:
  * the project's kernel-level bar: relative L2 <= 1e-4 (activations and the loss 1e-5);
  * elementwise: e(X) = max|X - X64| / max|X64|, e_hip <= max(M * e_aten, FLOOR).  One lost pixel of one weight-gradient element
    is 1.2e-4 .. 3.7e-3 in this measure and often below 1e-4 in relative L2 (tests/test_train_host.py pins that on the CPU).
M, FLOOR: see below PROBE_M.  Every case also asserts WHICH kernel ran (profile labels, pf_train_path_stats): a change of a
selector must not silently empty a case.  Every case writes its distances and kernels to train_layer_probe_dist.json in the
suite's scratch report directory (tests/helpers.py: probe_record); the run on MI355X is kept as profiles/train_layer_probe_dist.json.

Checked once each with a deliberate wrong-value edit (values only, not kept): wgrad_taps_kernel skipping the matrix work of every
item in the last column tile -> the 14 cases here that run it at 70 / 72 columns fail, tests/test_gpu_train.py's mini network
(no layer wider than 36 pixels) passes in all its variants; zero_stuff_kernel reading dy one column to the right -> the 7 stride-2
cases here fail, the mini network (its only stride-2 conv reads the input) passes.

Found by the BatchNorm cases at the end of this file (and fixed with them; this one needed no deliberate edit):
bn_stats_partial4_kernel, the statistics kernel every layer of the real network runs, summed each quad's x and x^2 in fp32 before
widening.  With |mean| / std ~ 270 per channel that kernel fails the four cases that run it (rvar L at e_hip 1.1e-3 / 5.6e-4 /
5.5e-4 / 4.2e-5 against e_aten 2.0e-6 / 2.6e-6 / 4.3e-6 / 1.8e-7, 44 .. 560 x; act L up to 22 x, dgamma L up to 49 x, grad a up to
44 x) while the pitched case on the scalar kernel and every case on randn data pass; widening the squares alone leaves it failing
(var = E[x^2] - mean^2 takes an error d of the mean as 2 mean d: tests/test_train_host.py), widening both brings every quantity
to 0.1 .. 1.5 x fp32 ATen.  No case before these had a channel with |mean| / std above a few units."""
import pytest
import torch

from tests.helpers import (MiniTrain, Probe, probe_distances, probe_failures, probe_mean_over_std, probe_record, probe_reference)

pytestmark = pytest.mark.gpu

# FLOOR = 2^-20, eight fp32 epsilons of the tensor's largest element: below that e_aten is luck (it is 3e-9 .. 2e-7 for the loss), not
# a measure of rounding.  M = the smallest power of two >= 2 x the worst e_hip / max(e_aten, FLOOR) measured on MI355X over all 81
# steps and every tensor of this file (profiles/train_layer_probe_dist.json): the worst ratio is 0.875 (grad a of the stride-2
# layer with two ranges at 33 x 68: e_hip 1.33e-6, e_aten 1.52e-6; the largest e_hip under the floor is 7.4e-7, act L of the
# 639-term 3x3 layer summed as one fp32 chain, train_blocked_sum = 0), so M = 2.  The caps of the checker (tests/helpers.py) are
# M <= 32, FLOOR <= 2e-5; with (2, 2^-20) the bar on dW is 1e-6 .. 3.4e-6, forty times below the smallest lost-pixel error.
# (Since the 4-wide BatchNorm statistics are summed in fp64 the figures of every case moved in their last digits: over the 89 steps
# the file has now, ill-conditioned cases aside, the worst ratio is 1.16 - dw L of the 1x1 layer 5 -> 3 at 9 x 72, e_hip 1.11e-6,
# e_aten 8.9e-7, floor 9.5e-7 - then 1.01, grad a of the BN case at 131 x 130.  M stays 2, which is now tighter than the rule.)
PROBE_M, PROBE_FLOOR = 2.0, 2.0 ** -20
# The cases with ill-conditioned channel statistics (BN below, cond='ill') get an M of their own BY THE SAME RULE: the smallest power
# of two >= 2 x the worst e_hip / max(e_aten, FLOOR) measured on MI355X over those cases and every tensor of them, at most
# PROBE_M_CAP (tests/helpers.py).  The worst ratio there is 1.53 (dbeta L of the slot case: e_hip 5.15e-5, e_aten 3.36e-5; the
# running variance, the quantity these cases are for, is at 0.12 .. 1.11, act L at 0.49 .. 1.00, dgamma L at 0.27 .. 0.87), so
# M = 4.  tests/test_train_host.py pins on the CPU that fp32 quad sums miss the bar on the running variance by 5x even at M = 32.
# (The well-conditioned BN cases keep PROBE_M = 2 as given; their worst ratio is 1.01, grad a at 131 x 130.)
PROBE_M_ILL = 4.0

DEFAULTS = {'wgrad_taps': 1, 'train_forward_s4': 0, 'train_blocked_sum': 1}


def _kernels(labels):
    """the kernels of interest of a profile, without the per-layer tag of the weight gradients (a BatchNorm / bias launch is
    labelled with its two kernels, 'first+second')"""
    keep = ('wgrad_', 'conv_dma_kernel', 'conv_s4', 'ce_fwd_bwd', 'zero_stuff', 'bn_', 'bias_bwd')
    out = set()
    for lab in labels:
        lab = lab.split(' @')[0].replace('void pf::', '').replace('(pf::ConvArgs)', '')
        if any(k in lab for k in keep) and 'reduce' not in lab:
            out.add(lab)
    return sorted(out)


def _run(case, tag='', force=None, m=PROBE_M, rel_l2=True, keep=None, **options):
    """one training step of the case on the device -> (kernels that ran, path statistics); the comparison with the references, both
    criteria (``rel_l2=False``: the elementwise one alone, tests/helpers.py: probe_failures), is asserted here.  ``keep``: a
    dict that receives the device's quantities"""
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    params, x, lab = case.data()
    for k, v in options.items():
        assert k in DEFAULTS
        pflib.check(L.pf_set_option(k.encode(), v), 'pf_set_option')
    if force:
        pflib.check(L.pf_debug_force_conv(1, force[0], force[1], 0), 'pf_debug_force_conv')
    net = None
    try:
        net = MiniTrain(case.spec(), params)
        before = L.pf_last_error()
        pflib.profile(True)
        try:
            loss = net.step(x.cuda(), lab.cuda())
            kernels = _kernels(r['label'] for r in pflib.profile_results())
        finally:
            pflib.profile(False)
        assert L.pf_last_error() == before, L.pf_last_error()
        got = case.quantities_hip(net, loss)
        stats = net.path_stats()
    finally:
        if net is not None:
            net.close()
        for k, v in DEFAULTS.items():
            L.pf_set_option(k.encode(), v)
        L.pf_debug_force_conv(0, 0, 0, 0)
    r64, r32 = probe_reference(case)
    dist = probe_distances(got, r64, r32)
    probe_record(case.name + tag, dist, kernels)
    print(case.name + tag, {k: 'e_hip %.2e e_aten %.2e rel %.2e' % (d['e_hip'], d['e_aten'], d['rel_hip']) for k, d in dist.items()})
    print('   kernels:', kernels, 'path stats:', stats)
    assert stats[6] == 0, stats                  # no launch of the generic (register-staged) kernel
    if keep is not None:
        keep.update(got)
    bad = probe_failures(dist, m, PROBE_FLOOR, rel_l2)
    assert not bad, bad
    return kernels, stats


def _ids(cases):
    return [c[0].name for c in cases]


# ------------------------------------------------------------------------------------------------ wgrad_taps, all 12 instantiations
# T = 6 / 11 / 18 <- 10 / 18 / 28 outputs per chunk; NC = 1 <- 12 inputs, NC = 2 <- 40 (the second group of 32 a quarter full);
# 10 x 20: the narrow items (32 pixels x R = 4 rows, 10 rows = 2.5 items); 9 x 72: the wide ones, two column tiles (64 + 8), odd height
_T_OF = {10: 6, 18: 11, 28: 18}
TAPS = [(Probe('taps %d->%d %dx%d' % (cin, cout, h, w), 3, 1, [('a', 0, cin)], cout, (h, w), cin),
         'wgrad_taps_kernel<%d, %d, %d, %d>' % (_T_OF[cout], 1 if cin <= 16 else 2, 32 if w <= 32 else 64, 4 if w <= 32 else 2))
        for cout in (10, 18, 28) for cin in (12, 40) for h, w in ((10, 20), (9, 72))]
TAPS += [
    # several cout chunks: 46 = 2 x 23, 70 = 24 + 24 + 22 (a partial last chunk)
    (Probe('taps 40->46 9x72', 3, 1, [('a', 0, 40)], 46, (9, 72), 40), 'wgrad_taps_kernel<18, 2, 64, 2>'),
    (Probe('taps 40->70 9x72', 3, 1, [('a', 0, 40)], 70, (9, 72), 40), 'wgrad_taps_kernel<18, 2, 64, 2>'),
    # many items per workgroup (the double-buffered loop, one barrier per item): 3 chunks x 9 cin groups = 27 tiles -> 9 slabs, 36 items
    (Probe('taps 270->70 17x72', 3, 1, [('a', 0, 270)], 70, (17, 72), 270), 'wgrad_taps_kernel<18, 2, 64, 2>'),
    # two ranges from two tensors, L writing channels [10, 28) of a wider tensor
    (Probe('taps 12+28->18 slot 9x72', 3, 1, [('a', 0, 12), ('a2', 4, 28)], 18, (9, 72), 12, 32, slot=True), 'wgrad_taps_kernel<11, 2, 64, 2>'),
    (Probe('taps 40->18 9x72 b1', 3, 1, [('a', 0, 40)], 18, (9, 72), 40, b=1), 'wgrad_taps_kernel<11, 2, 64, 2>'),
]


@pytest.mark.parametrize('case,want', TAPS, ids=_ids(TAPS))
def test_wgrad_taps(case, want):
    kernels, _ = _run(case, wgrad_taps=2)
    assert want in kernels, kernels
    assert not any(k.startswith('wgrad_tiled_kernel<3') for k in kernels), kernels


# ------------------------------------------------------------------------------------------------ wgrad_tiled
TILED = [(Probe('tiled %d->%d %dx%d' % (cin, cout, h, w), 3, 1, [('a', 0, cin)], cout, (h, w), cin), 'wgrad_tiled_kernel<3, 1, 2>')
         for h, w in ((9, 72), (17, 136)) for cin, cout in ((12, 10), (40, 46), (50, 70))]     # a second / third 64-pixel segment per row
TILED += [
    (Probe('tiled 1x1 90->70 9x72', 1, 1, [('a', 0, 90)], 70, (9, 72), 90), 'wgrad_tiled_kernel<1, 1, 1>'),
    (Probe('tiled 1x1 5->3 9x72', 1, 1, [('a', 0, 5)], 3, (9, 72), 5), 'wgrad_tiled_kernel<1, 1, 1>'),
    (Probe('tiled s2 40->24 34x72', 3, 2, [('a', 0, 40)], 24, (34, 72), 40), 'wgrad_tiled_kernel<3, 2, 1>'),
]


@pytest.mark.parametrize('case,want', TILED, ids=_ids(TILED))
def test_wgrad_tiled(case, want):
    kernels, _ = _run(case, wgrad_taps=0)
    assert want in kernels, kernels
    assert not any(k.startswith('wgrad_taps') or k.startswith('wgrad_partial') for k in kernels), kernels
    if case.stride == 2:
        assert 'zero_stuff_kernel' in kernels, kernels       # L reads a, not the input: its backward-data pass runs


# ------------------------------------------------------------------------------------------------ wgrad_partial (the gather form)
PARTIAL = [
    (Probe('partial s2 40->24 35x70', 3, 2, [('a', 0, 40)], 24, (35, 70), 40), 'wgrad_partial_kernel<3, 2>'),
    (Probe('partial s2 12->40 35x70', 3, 2, [('a', 0, 12)], 40, (35, 70), 12), 'wgrad_partial_kernel<3, 2>'),
    (Probe('partial s2 12->40 33x68', 3, 2, [('a', 0, 12)], 40, (33, 68), 12), 'wgrad_partial_kernel<3, 2>'),     # Win % 4 == 0, Wout % 4 != 0
]


@pytest.mark.parametrize('case,want', PARTIAL, ids=_ids(PARTIAL))
def test_wgrad_partial(case, want):
    kernels, _ = _run(case)
    assert want in kernels and 'zero_stuff_kernel' in kernels, kernels
    assert not any(k.startswith('wgrad_tiled_kernel<3, 2') for k in kernels), kernels


# ------------------------------------------------------------------------------------------------ stride-2 backward-data, two ranges
# zero-stuffing + the flipped stride-1 convolution per range, from a tensor that is not the input (the one-range forms are the
# stride-2 cases above).  The second range overlaps the first one in a: the first range's gradient is stored, the second's added
S2_TWO = [
    (Probe('s2 two ranges 28+12->24 34x72', 3, 2, [('a', 0, 28), ('a', 12, 12)], 24, (34, 72), 40), 'wgrad_tiled_kernel<3, 2, 1>'),
    (Probe('s2 two ranges 28+12->24 35x70', 3, 2, [('a', 0, 28), ('a', 12, 12)], 24, (35, 70), 40, bn=False), 'wgrad_partial_kernel<3, 2>'),
    (Probe('s2 two ranges 20+8->40 33x68', 3, 2, [('a2', 2, 20), ('a', 3, 8)], 40, (33, 68), 12, 24), 'wgrad_partial_kernel<3, 2>'),
]


@pytest.mark.parametrize('case,want', S2_TWO, ids=_ids(S2_TWO))
def test_stride2_backward_data_two_ranges(case, want):
    kernels, _ = _run(case)
    assert want in kernels and 'zero_stuff_kernel' in kernels, kernels
    # the backward-data convolutions are stride-1 3x3 conv_dma launches with blocked sums
    assert any(k.startswith('conv_dma_kernel<3, 1,') and k.endswith(', 1>') for k in kernels), kernels


# ------------------------------------------------------------------------------------------------ odd widths at two column tiles
# 9 x 70, rows padded to 72: gathered input, conv + BatchNorm output kept in padded rows, ONE backward-data conv over all ranges,
# scattered back to three ranges of two tensors.  With fin reading a[4:10] as well, those channels of a's gradient are written
# before L's pass: L's first range is ADDED (its other channels cleared beforehand), the other two stored, by one launch of
# unpad_scatter_multi.  The first case has its third range overlap the first one in a instead: the first stored, the third added
# to it - which one launch did in no defined order (grad a 0.49 off in relative L2 before the schedule gave such ranges a launch each)
_ODD_SRCS = [('a', 0, 16), ('a2', 2, 10), ('a', 16, 8)]
ODD = [
    (Probe('odd 3x3 40->18 9x70 overlap', 3, 1, [('a', 0, 16), ('a2', 2, 10), ('a', 8, 14)], 18, (9, 70), 24, 12), 0, 'wgrad_tiled_kernel<3, 1, 2>'),
    (Probe('odd 3x3 40->18 9x70', 3, 1, _ODD_SRCS, 18, (9, 70), 24, 12, fin_a=(4, 6)), 0, 'wgrad_tiled_kernel<3, 1, 2>'),
    (Probe('odd 3x3 40->18 9x70 taps', 3, 1, _ODD_SRCS, 18, (9, 70), 24, 12, fin_a=(4, 6)), 2, 'wgrad_taps_kernel<11, 2, 64, 2>'),
    (Probe('odd 1x1 40->18 9x70', 1, 1, _ODD_SRCS, 18, (9, 70), 24, 12, fin_a=(4, 6)), 0, 'wgrad_tiled_kernel<1, 1, 1>'),
]


@pytest.mark.parametrize('case,taps,want', ODD, ids=_ids(ODD))
def test_odd_width_two_column_tiles(case, taps, want):
    kernels, stats = _run(case, wgrad_taps=taps)
    assert want in kernels, kernels
    assert not any(k.startswith('wgrad_partial') for k in kernels), kernels
    # a, a2, L and fin read gathered copies; a, a2 and L keep their outputs in padded rows; L and fin (at least): ONE backward-data
    # conv over all ranges, scattered by unpad_scatter_multi
    assert stats[3] >= 4 and stats[4] == 3 and stats[5] >= 2, stats


# ------------------------------------------------------------------------------------------------ forced conv_dma shapes
# pf_debug_force_conv(1, wm, nt, 0) in the training schedule: the 10 built (wm, nt) shapes x blocked sums on / off.  Layers at 20 x 40:
# a three-range 3x3 layer 71 -> 37 (ranges of 49, 12 and 10 channels: K tails, three cout tiles forward, four / one / one backward)
# behind a = 6 -> 50 (four cout tiles, a K tail), and a 1x1 layer 45 -> 70 (five cout tiles forward, three backward)
CONV3 = Probe('conv_dma 3x3 49+12+10->37 20x40', 3, 1, [('a', 0, 49), ('a2', 2, 12), ('a', 40, 10)], 37, (20, 40), 50, 16)
CONV1 = Probe('conv_dma 1x1 45->70 20x40', 1, 1, [('a', 0, 45)], 70, (20, 40), 45)
SHAPES = [(4, 1), (4, 2), (4, 3), (4, 4), (2, 1), (2, 2), (2, 3), (2, 4), (1, 1), (1, 2)]


@pytest.mark.parametrize('kacc', [1, 0])
@pytest.mark.parametrize('wm,nt', SHAPES)
def test_forced_conv_dma_shapes_in_training(wm, nt, kacc):
    tag = ' wm%d nt%d kacc%d' % (wm, nt, kacc)
    k3, s3 = _run(CONV3, tag, force=(wm, nt), wgrad_taps=0, train_blocked_sum=kacc)
    # a: four cout tiles - the forced shape itself; L forward: min(nt, 3); its backward-data convs: min(nt, 4), 1, 1
    tail = ', 0, 0, 1>' if kacc else ', 0, 0>'
    for n in {nt, min(nt, 3), 1}:
        assert 'conv_dma_kernel<3, 1, %d, %d, %d%s' % (wm, 4 // wm, n, tail) in k3, (n, k3)
    assert not any(k.startswith('conv_dma_kernel<3') and not k.startswith('conv_dma_kernel<3, 1, %d, %d,' % (wm, 4 // wm)) for k in k3), k3
    assert all(k.endswith(tail) for k in k3 if k.startswith('conv_dma_kernel<3')), k3
    assert 'conv_dma_kernel<1, 1, %d, %d, 1, 0, 0>' % (wm, 4 // wm) in k3, k3        # fin: 37 -> 11, one cout tile
    assert s3[0] == 0 and s3[1] == 0 and s3[2] == 0, s3       # a forced shape is no table / cost-model / measured choice
    k1, s1 = _run(CONV1, tag, force=(wm, nt), wgrad_taps=0, train_blocked_sum=kacc)
    for n in {nt, min(nt, 3)}:                                # forward: five cout tiles; backward-data (45 channels): three
        assert 'conv_dma_kernel<1, 1, %d, %d, %d, 0, 0>' % (wm, 4 // wm, n) in k1, (n, k1)
    assert s1[0] == 0 and s1[1] == 0 and s1[2] == 0, s1


# ------------------------------------------------------------------------------------------------ loss head: 19 classes, uint8 labels
HEAD = Probe('head 19 classes u8 dead image 12->10 10x20', 3, 1, [('a', 0, 12)], 10, (10, 20), 12, n_cls=19, u8=True, dead=True)


def test_loss_head_19_classes_uint8_labels_and_an_image_without_labels():
    kernels, _ = _run(HEAD)
    assert 'ce_fwd_bwd_kernel<19>' in kernels, kernels
    _, _, lab = HEAD.data()
    assert lab.dtype == torch.uint8 and bool((lab[0] == 255).all()) and bool((lab[1] != 255).any())


# ------------------------------------------------------------------------------------------------ forward on the packed-pair kernels
S4 = [TAPS[0][0], ODD[1][0], TAPS[15][0], TILED[6][0]]       # narrow 12 -> 10; odd width, three ranges; the slot at channel 10; 1x1 90 -> 70


@pytest.mark.parametrize('case', S4, ids=[c.name for c in S4])
def test_forward_on_packed_pairs(case):
    kernels, stats = _run(case, ' s4', train_forward_s4=1)
    assert stats[7] == 1 + int(case.slot), stats              # L (and side); a / a2 read the dense input, fin has no BatchNorm
    assert any('conv_s4' in k for k in kernels), kernels


# ------------------------------------------------------------------------------------------------ BatchNorm at hard statistics
# Every case above is randn weights on randn input: |mean| / std of L's conv output is of order 1 in every channel, and no plane is
# large enough for a block of a (channel, 64 slabs) x 256 reduction to make a second trip of its slab loop.  Here L is a 1x1 conv +
# BatchNorm (tests/helpers.py: Probe, cond / rstats) and the cases are
#   ill:   every channel of y at |mean| / std ~ 300 (asserted on the float64 reference: the case must stay what it is for) - what a
#          layer sees that reads post-ReLU activations through same-sign weights.  The fixed relative-L2 bars are left out
#          (probe_failures says why), M is PROBE_M_ILL;
#   wrap:  today's data on planes of 132 x 508 (16764 quads: slab 0 of the 4-wide forms makes a second, partly filled trip; also
#          bias_bwd_kernel's wrap, per plane, for fin) and 131 x 130 with one image (17030 elements, W % 4 = 2: the scalar forms on
#          pitched rows);
#   degenerate: channels with y = 0 (var = 0) and with var << eps.
# The running statistics the step writes are compared in all of them (they start at 0: 0.1 x the batch statistic).
BN_FWD4, BN_FWD1 = 'bn_stats_partial4_kernel+bn_apply_relu4_kernel', 'bn_stats_partial_kernel+bn_apply_relu_kernel'
BN_BWD4, BN_BWD_PITCH = 'bn_bwd_partial4_kernel+bn_bwd_apply4_kernel', 'bn_bwd_partial_kernel+bn_bwd_apply_pitch_kernel'
BIAS_BWD = 'bias_bwd_kernel+bias_bwd_final_kernel'
BN = [
    (Probe('bn ill 12->10 10x20', 1, 1, [('a', 0, 12)], 10, (10, 20), 12, cond='ill', rstats=True), (BN_FWD4, BN_BWD4)),     # 50 quads: slab 0 alone
    (Probe('bn ill 40->18 9x72', 1, 1, [('a', 0, 40)], 18, (9, 72), 40, cond='ill', rstats=True), (BN_FWD4, BN_BWD4)),
    (Probe('bn ill 12->10 9x70', 1, 1, [('a', 0, 12)], 10, (9, 70), 12, cond='ill', rstats=True), (BN_FWD1, BN_BWD_PITCH)),   # rows of 72
    # L writes channels [10, 28) of a 28-channel tensor: dst_choff / t_ctotal of the 4-wide apply and backward kernels
    (Probe('bn ill 40->18 slot 9x72', 1, 1, [('a', 0, 40)], 18, (9, 72), 40, slot=True, cond='ill', rstats=True), (BN_FWD4, BN_BWD4)),
    (Probe('bn wrap 12->10 132x508', 1, 1, [('a', 0, 12)], 10, (132, 508), 12, rstats=True), (BN_FWD4, BN_BWD4)),
    (Probe('bn wrap 12->10 131x130 b1', 1, 1, [('a', 0, 12)], 10, (131, 130), 12, b=1, rstats=True), (BN_FWD1, BN_BWD_PITCH)),
    (Probe('bn ill 12->10 132x508', 1, 1, [('a', 0, 12)], 10, (132, 508), 12, cond='ill', rstats=True), (BN_FWD4, BN_BWD4)),  # long fp64 sums of large squares
    (Probe('bn degenerate 12->10 10x20', 1, 1, [('a', 0, 12)], 10, (10, 20), 12, cond='degenerate', rstats=True), (BN_FWD4, BN_BWD4)),
]


@pytest.mark.parametrize('case,forms', BN, ids=_ids(BN))
def test_batchnorm_at_hard_statistics(case, forms):
    ill = case.cond == 'ill'
    ratio = probe_mean_over_std(case)
    print(case.name, '|mean| / std of y per channel: min %.1f max %.1f' % (float(ratio.min()), float(ratio.max())))
    if ill:
        assert 200.0 <= float(ratio.min()) <= 500.0, ratio
    got = {}
    kernels, stats = _run(case, m=PROBE_M_ILL if ill else PROBE_M, rel_l2=not ill, keep=got)
    # every BatchNorm of the case (a, L, side) has the case's plane: all of them run the one form, fin the bias kernels
    assert {k for k in kernels if k.startswith('bn_')} == set(forms), kernels
    assert BIAS_BWD in kernels, kernels
    h, w = case.size
    assert stats[4] == (2 if w % 4 else 0), stats             # a and L keep their outputs in padded rows exactly where W % 4 != 0
    if forms[0] == BN_FWD4:
        assert h * w % 4 == 0 and (h * w // 4 > 16384) == ('132x508' in case.name)     # the 4-wide forms' wrap, where it is meant
    else:
        assert (case.b * h * w > 16384) == ('wrap' in case.name)                       # the scalar forms' wrap
    if case.cond == 'degenerate':
        params, _, _ = case.data()
        beta, act = params['L']['beta'].double(), got['act L']
        for c in (0, 1):         # y = 0: mean = var = 0, z = fma(0, gamma / sqrt(eps), beta - 0) = beta, xhat = 0
            assert torch.equal(act[:, c], beta[c].expand_as(act[:, c])), (c, act[:, c].unique(), beta[c])
            assert float(got['dgamma L'][c]) == 0.0 and float(got['rvar L'][c]) == 0.0 and float(got['rmean L'][c]) == 0.0, c
        y_var = got['rvar L'][2:4] / 0.1
        assert bool((y_var > 0).all()) and bool((y_var < 1e-5 * 1e-5).all()), y_var     # var << eps, and not flushed to 0
