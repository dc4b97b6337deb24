"""The fg forward under model.fg_arithmetic = 'fp16_pair' (PF_FG_PAIR: pair_kernel of csrc/fg_gemm.hip) against float64.

Single-kernel cases, bar D' (derived, elementwise): the bar D of tests/test_gpu_fg_stages.py plus the pair's own term,
    |hip - ref64| <= 1.01 ((2K + 2) 2^-24 + 2^-21) (op(|x|, |w|) + |b|)
2^-21 = 2^-23 per operand + 2^-22 for the dropped mid*mid product (tests/test_fg_pair_host.py pins it on the float64 emulation), through
the gate derivatives for a cell.  A cell whose inputs are not public outputs (the decoder's cells read the encoder's h and c) is checked
by carrying the bound along: `cell_bound` returns, next to the float64 state, what the kernel's own state may differ from it by.

Whole forwards, bar P' per tensor: max|hip - ref64| <= 4 max|ref32 - ref64| + 1e-6 (1 + max|ref64|) - the fp32 path's bar P with its
factor 2 doubled (DESIGN section 4 rates a pair operand about two bits narrower than fp32).  Every case prints err / e32 under -s and
records it in fg_pair_dist.json of the suite's report directory (the MI355X run is kept as profiles/fg_pair_dist.json).

A flags = 0 packed buffer handed to a PF_FG_PAIR forward is the caller's contract (include/pfhip.h) and is NOT tested: the pair section
lies behind the end of such a buffer, so the call reads out of bounds.  FGModel cannot make it: its caches are keyed on the arithmetic.
"""
import contextlib

import numpy as np
import os
import pytest
import torch
import torch.nn.functional as F

import fg_ref64 as R
from helpers import _merge_report

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
OUTS = ('normalized_trajectory', 'unnormalized_trajectory', 'mask_feats', 'output_feats', 'masks')
U = 2.0 ** -24
PAIR = 2.0 ** -21
HOT_GAIN = 16.0
ENC0, ENC1, DEC0, DEC1 = R._CELLS[0], R._CELLS[1], R._CELLS[2], R._CELLS[3]


def eps(K):
    return 1.01 * ((2 * K + 2) * U + PAIR)


def record(case_id, entry):
    _merge_report('fg_pair_dist.json', case_id, entry)


@pytest.fixture(scope='module')
def model():
    from panoptic_forecasting_amd.registry import build_model
    p = R.fg_params(fg_arithmetic='fp16_pair', fg_on_range='raise')      # a flagged forward fails its test instead of passing on fp32
    p['no_gpu'] = False
    m = build_model(p)
    m.load_state_dict(R.fill_weights(m.state_dict()))
    return m


@pytest.fixture(scope='module')
def base(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.fixture(scope='module')
def base64(base):
    return {k: v.double() for k, v in base.items()}


@pytest.fixture(scope='module', autouse=True)
def tf32_off():
    was = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = was


@contextlib.contextmanager
def mode(model, arithmetic=None, on_range=None):
    was = model.fg_arithmetic, model.fg_on_range
    model.fg_arithmetic = arithmetic or was[0]
    model.fg_on_range = on_range or was[1]
    try:
        yield model
    finally:
        model.fg_arithmetic, model.fg_on_range = was


@contextlib.contextmanager
def loaded(model, base, sd):
    """the tensors of ``sd`` that are not the base fill's in the model, the base fill back on the way out"""
    new = {k: v for k, v in sd.items() if v is not base[k]}
    model.load_state_dict(new, strict=False)
    try:
        yield sd
    finally:
        model.load_state_dict({k: base[k] for k in new}, strict=False)


def transparent(sd, base, cell):
    """fg_ref64.crafted's 'transparent_cell1' for any layer-1 cell, with b_f = -100: sigm(-100) = 1 / (1 + inf) = 0 in fp32, the cell
    forgets its state: h' = s(20) tanh(s(20) tanh(x)), s(20) = 1 in fp32"""
    w = torch.zeros_like(base[cell + '.weight'])
    w[768:, :256, 1, 1] = torch.eye(256, device=w.device)
    b = torch.zeros_like(base[cell + '.bias'])
    b[:256] = 20
    b[256:512] = -100
    b[512:768] = 20
    sd[cell + '.weight'], sd[cell + '.bias'] = w, b
    return sd


def _args(case, n, t_in, t_out, classes=None, **kw):
    inputs, labels = R.make_inputs(case, [n], t_in=t_in, t_out=t_out, **kw)
    a = [x.to(DEV) if torch.is_tensor(x) else x for x in R.forward_args(inputs, labels)]
    if classes is not None:
        a[8] = torch.as_tensor(classes, dtype=torch.long, device=DEV)
    return a


def _copies(masks):
    n = masks.size(0)
    return masks.reshape(n, 14, 2, 14, 2).permute(0, 1, 3, 2, 4).reshape(n, 14, 14, 4)


def _ratio(got, ref, bar):
    err = (got.double() - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------ one kernel at a time, bar D'
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('pos,chans', [(1, R.ONEHOT_A), (4, R.ONEHOT_B)], ids=['fcn1-A', 'fcn4-B'])
def test_fcn_3x3_relu_alone(model, base, pos, chans, n):
    """pair_kernel<relu>: mask_fcn<pos> from the base fill, the other three identities, the deconvolution a replication, the predictor
    a selection of channel chans[class]; the classes rotate over the forwards so that all eight columns of the set are seen at every N.
    An identity layer on the pair path hands on hi + mid, x to within 2^-23 |x| (and itself from then on), not x bit for bit as on
    the fp32 path: what stands in front of the layer moves its input by that much, what stands behind it its output; the bar is the
    issue's, unchanged (the measured ratios are ~1e-4 of it)."""
    K = 256 * 9
    sd = R.crafted(base, [('ident_fcn', k) for k in (1, 2, 3, 4) if k != pos] + ['replicate_deconv', ('onehot_predictor', chans)])
    worst, top = 0.0, 0.0
    with loaded(model, base, sd):
        for first in range(0, 8, n):
            classes = [(first + j) % 8 for j in range(n)]
            args = _args(30 + pos, n, 1, 1, classes=classes)
            out = model(*args)
            cp = _copies(out['masks'])
            for j in (1, 2, 3):
                assert torch.equal(cp[..., j], cp[..., 0]), 'the four (dy, dx) copies differ'
            x = out['output_feats'].double()
            if pos != 1:
                x = F.relu(x)
            w, b = sd['mask_head.mask_fcn%d.weight' % pos].double(), sd['mask_head.mask_fcn%d.bias' % pos].double()
            ch = torch.tensor(chans, device=DEV)[args[8]]
            rows = torch.arange(n, device=DEV)
            ref = F.relu(F.conv2d(x, w, b, padding=1))[rows, ch]
            bar = eps(K) * F.conv2d(x.abs(), w.abs(), b.abs(), padding=1)[rows, ch]
            worst = max(worst, _ratio(cp[..., 0], ref, bar))
            top = max(top, float(ref.abs().max()))
    print('pair mask_fcn%d, N = %d: worst err / bar D\' = %.4g (K = %d, max|ref| %.3g)' % (pos, n, worst, K, top))
    record('fcn%d N=%d' % (pos, n), {'err_over_bar': float('%.4g' % worst), 'K': K})
    assert top > 0.1 and worst <= 1.0


def _slack(fn, pre):
    """twice the distance of torch's fp32 evaluation of ``fn`` from float64 on the float64 pre-activations rounded to fp32 (it stands
    for the kernel's __expf / tanhf, as in test_gpu_fg_stages.test_first_cell_alone)"""
    return 2 * float((fn(*[p.float() for p in pre]).double() - fn(*pre)).abs().max())


def cell_bound(sd, cell, x, dx, h, dh, c, dc, first):
    """One cell in float64 on the reference inputs x, h, c -> (h', c', dh', dc'): d* bound what the kernel's own tensors differ from
    the float64 ones by, given the same for its inputs.  Pre-activations: the kernel's sum over its own inputs (within dx, dh of the
    reference's) errs by eps(K) op(|x| + dx, |w|, |b|), and its inputs' error enters through |w|.  Gates: sigmoid is 1/4-Lipschitz and
    <= 1, tanh 1-Lipschitz and <= 1, so |dc'| <= sf (df (|c| + dc) + dc) + di/4 + dg with sf = sigmoid(f + df) >= both the forget gate
    and its slope anywhere within df of f (s' = s (1 - s) <= s; a cell with b_f = -100 forgets exactly), and |dh'| <= do/4 + dc'
    (first step: c = dc = 0 and the h half of K is never read)."""
    w, b = sd[cell + '.weight'].double(), sd[cell + '.bias'].double()
    cin = x.size(1)
    if first:
        w = w[:, :cin]
        xin, dxin = x, dx
    else:
        xin, dxin = torch.cat([x, h], 1), torch.cat([dx, dh], 1)
    K = xin.size(1) * 9
    pre = F.conv2d(xin, w, b, padding=1).chunk(4, 1)
    dpre = (eps(K) * F.conv2d(xin.abs() + dxin, w.abs(), b.abs(), padding=1) + F.conv2d(dxin, w.abs(), padding=1)).chunk(4, 1)
    i, f, o, g = pre
    di, df, do, dg = dpre
    cfn = lambda i, f, g: torch.sigmoid(f) * c.to(f.dtype) + torch.sigmoid(i) * torch.tanh(g)
    hfn = lambda i, f, o, g: torch.sigmoid(o) * torch.tanh(cfn(i, f, g))
    c2 = cfn(i, f, g)
    h2 = hfn(i, f, o, g)
    sf = torch.sigmoid(f + df)
    dc2 = sf * (df * (c.abs() + dc) + dc) + 0.25 * di + dg + _slack(cfn, (i, f, g))
    dh2 = 0.25 * do + dc2 + _slack(hfn, (i, f, o, g))
    return h2, c2, dh2, dc2, K


def _vec(sd, n):
    return sd['traj_feat_out.bias'].double()[None, :, None, None].expand(n, -1, 14, 14)


@pytest.mark.parametrize('n', [1, 3])
def test_first_cell_alone(model, base, n):
    """pair_kernel<lstm> with h == nullptr and the vec source (K = 272 * 9: 17 rounds, the first one all vec), as
    test_gpu_fg_stages.test_first_cell_alone: mask_feats[:, 0] = tanh(tanh(h0)) through the transparent layer 1 and the identity out conv."""
    args = _args(38, n, 1, 1)
    sd = transparent(R.crafted(base, ['ident_out_conv', ('const_traj_feat', 1.5)]), base, ENC1)
    with loaded(model, base, sd):
        got = model(*args)['mask_feats'][:, 0].clone()
    with torch.no_grad():
        z = torch.zeros(n, 256, 14, 14, dtype=torch.float64, device=DEV)
        x = torch.cat([_vec(sd, n), args[3][:, 0].double()], 1)
        h0, c0, dh0, dc0, K = cell_bound(sd, ENC0, x, torch.zeros_like(x), z, z, z, z, True)
        h1, _, dh1, _, _ = cell_bound(sd, ENC1, h0, dh0, z, z, z, z, True)
        ref = R.forward64(sd, *args)['mask_feats'][:, 0]
    assert K == 272 * 9 and float((h1 - ref).abs().max()) < 1e-12
    r = float(((got.double() - ref).abs() / dh1).max())
    print('pair first cell, N = %d: worst err / bar = %.4g (max err %.3g, max bar %.3g)' % (n, r, float((got.double() - ref).abs().max()), float(dh1.max())))
    record('first cell N=%d' % n, {'err_over_bar': float('%.4g' % r), 'K': K})
    assert float(ref.abs().max()) > 0.3 and r <= 1.0


T64 = float(np.tanh(1.0))
T_TOL = 2.0 ** -22            # tanhf(1.0f) on the device: within 4 ulp of the float64 value rounded to fp32


def switch_cell(sd, base, cell, src, gain):
    """A cell whose state is known without computing it: every weight 0 except W_o[j][src + j] = gain at the centre tap, b_i = b_g = 100,
    b_f = b_o = -100.  In fp32, sigm(100) = 1 / (1 + 0) = 1, sigm(-100) = 1 / (1 + inf) = 0, tanhf(100) = 1, so c' = 1 and
    h' = s(gain u_j - 100) tanhf(1): with a source plane u of values 0 and >= 150 / gain, h' is 0 or tanhf(1.0f) exactly."""
    w = torch.zeros_like(base[cell + '.weight'])
    j = torch.arange(256, device=w.device)
    w[512 + j, src + j, 1, 1] = gain
    b = torch.full_like(base[cell + '.bias'], -100.0)
    b[:256] = 100
    b[768:] = 100
    sd[cell + '.weight'], sd[cell + '.bias'] = w, b
    return sd


def _is_switch_output(t, pattern):
    """t = pattern * tanhf(1.0f): zeros where the pattern is 0, one single value within T_TOL of tanh(1) where it is 1"""
    on = t[pattern > 0]
    return bool((t[pattern == 0] == 0).all()) and bool((on == on[0]).all()) and abs(float(on[0]) - T64) <= T_TOL * T64


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('which', ['dec0', 'dec1'])
def test_decoder_cells(model, base, which, n):
    """The K = 528 * 9 kernel (a second-step layer-0 cell: vec, x and h all read) and the K = 512 * 9 one (a layer-1 cell: x and h, no
    vec) from the base fill, each with every input known.  One input and one output step, binary input features b (0 / 1), identity out
    convs - mask_feats[:, 0] is the encoder's h1 and mask_feats[:, 1] the decoder's, bit for bit - and the constant trajectory
    features.  The encoder's layer-0 cell is a switch_cell on the features: h0 = b T, c0 = 1, T = tanhf(1.0f), the one number not known
    to the last bit (T_TOL: it enters the bar as an input error, through |w|).
      'dec0'  the decoder's layer-0 cell reads vec, x = mask_feats[:, 0] (the kernel's own input; the encoder's layer 1 from the base
              fill makes it a real-valued plane), h = b T, c = 1; its h' is seen through a transparent layer 1: tanh(tanh(h')).
      'dec1'  both layer-0 cells and the encoder's layer 1 are switch cells (the encoder's layer 1 negated: (1 - b) T), so the decoder's
              layer-1 cell reads x = b T, h = mask_feats[:, 0] = (1 - b) T - different planes: swapped halves cannot pass - and c = 1."""
    args = _args(43, n, 1, 1)
    args[3] = (args[3] > 0.5).float()
    b = args[3][:, 0].double()
    sd = switch_cell(R.crafted(base, ['ident_out_conv', ('const_traj_feat', 1.5)]), base, ENC0, 16, 200.0)
    if which == 'dec0':
        sd = transparent(sd, base, DEC1)
    else:
        sd = switch_cell(switch_cell(sd, base, DEC0, 272, 200.0), base, ENC1, 0, -400.0)
        sd[ENC1 + '.bias'] = sd[ENC1 + '.bias'].clone()
        sd[ENC1 + '.bias'][512:768] = 100                     # o = 100 - 400 T b: the negated plane
    with loaded(model, base, sd):
        mf = model(*args)['mask_feats'].clone()
    with torch.no_grad():
        z = torch.zeros(n, 256, 14, 14, dtype=torch.float64, device=DEV)
        one = torch.ones_like(z)
        cmf = mf[:, 0].double()
        h0, dh0 = b * T64, b * T64 * T_TOL
        if which == 'dec0':
            _, c1, _, dc1, _ = cell_bound(sd, ENC1, h0, dh0, z, z, z, z, True)
            x = torch.cat([_vec(sd, n), cmf], 1)
            h0d, _, dh0d, _, K = cell_bound(sd, DEC0, x, torch.zeros_like(x), h0, dh0, one, z, False)
            ref, _, bar, _, _ = cell_bound(sd, DEC1, h0d, dh0d, cmf, z, c1, dc1, False)
            assert K == 528 * 9
        else:
            assert _is_switch_output(mf[:, 0], 1 - b)
            ref, _, bar, _, K = cell_bound(sd, DEC1, h0, dh0, cmf, z, one, z, False)
            assert K == 512 * 9
    err = (mf[:, 1].double() - ref).abs()
    r = float((err / bar).max())
    print('pair %s, N = %d: worst err / bar = %.4g (K = %d, max err %.3g, max bar %.3g, max|ref| %.3g)'
          % (which, n, r, K, float(err.max()), float(bar.max()), float(ref.abs().max())))
    record('%s N=%d' % (which, n), {'err_over_bar': float('%.4g' % r), 'K': K, 'max_bar': float('%.4g' % float(bar.max()))})
    assert float(ref.abs().max()) > 0.1 and float(cmf.abs().max()) > 0.1 and r <= 1.0


def test_all_zero_weights_pack_and_run(model, base):
    """an all-zero weight tensor: k = 0, no division by zero, the layer's output is relu(bias) exactly - which the identity layers
    behind it hand on as hi + mid (22 significant bits; idempotent from then on)"""
    n = 2
    sd = R.crafted(base, [('ident_fcn', k) for k in (2, 3, 4)] + ['replicate_deconv', ('onehot_predictor', R.ONEHOT_A)])
    sd['mask_head.mask_fcn1.weight'] = torch.zeros_like(base['mask_head.mask_fcn1.weight'])
    args = _args(44, n, 1, 1, classes=[2, 5])
    with loaded(model, base, sd):
        out = model(*args)['masks'].clone()
    ch = torch.tensor(R.ONEHOT_A, device=DEV)[args[8]]
    v = F.relu(base['mask_head.mask_fcn1.bias'][ch])
    hi = v.half().float()
    want = (hi + (v - hi).half().float())[:, None, None].expand(-1, 28, 28)
    assert float(want.max()) > 0 and torch.equal(out, want)


# ------------------------------------------------------------------------------------------------------ whole forwards, bar P'
def _check(case_id, got, r64, r32):
    entry, bad = {}, []
    for k in got:
        e32 = float((r32[k].double() - r64[k]).abs().max())
        err = float((got[k].double() - r64[k]).abs().max())
        bar = 4 * e32 + 1e-6 * (1 + float(r64[k].abs().max()))
        entry[k] = {'err': float('%.4g' % err), 'e32': float('%.4g' % e32), 'err_over_e32': float('%.4g' % (err / e32 if e32 else 0.0)),
                    'err_over_bar': float('%.4g' % (err / bar))}
        assert bool(torch.isfinite(got[k]).all()), k
        if not err <= bar:
            bad.append((k, err, bar))
    print('%s: err / e32 per tensor %s' % (case_id, {k: v['err_over_e32'] for k, v in entry.items()}))
    record(case_id, entry)
    return bad


@pytest.mark.parametrize('n,t_in,t_out', [(1, 1, 1), (1, 3, 3), (3, 2, 1), (37, 3, 3), (5, 16, 2)])
def test_forward_against_float64(model, base, base64, n, t_in, t_out):
    args = _args(50 + t_in + t_out, n, t_in, t_out)
    out = model(*args)
    assert model.fg_status() == 0
    with torch.no_grad():
        r64 = R.forward64(base64, *args)
        r32 = R.forward64(base, *args, dtype=torch.float32)
    bad = _check('forward %d/%d/%d' % (n, t_in, t_out), {k: out[k] for k in OUTS}, r64, r32)
    assert not bad, bad


def test_saturated_gates(model, base):
    """test_gpu_fg_stages.test_saturated_gates' gain-16 case on the pair path"""
    args = _args(39, 4, 3, 3)
    taps = {}
    sd = R.crafted(base, ('hot', HOT_GAIN))
    with loaded(model, base, sd):
        out = model(*args)
        out = {k: out[k].clone() for k in OUTS}
    with torch.no_grad():
        r64 = R.forward64(sd, *args, taps=taps)
        r32 = R.forward64(sd, *args, dtype=torch.float32)
    share, top = R.saturation(taps['cell0_pre'][0])
    assert share >= 0.05 and top > 20.0
    bad = _check('hot gain %g' % HOT_GAIN, out, r64, r32)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------ maps
@pytest.mark.parametrize('method,key', [('predict_panoptic', 'seg_pan'), ('predict_semantics', 'seg_sem')])
def test_predict_matches_the_reference_map(model, golden_dir, method, key):
    fx = np.load(os.path.join(golden_dir, 'g8_fgnet.npz'))
    counts = list(fx['counts'])
    inputs, labels = R.make_inputs(0, counts)
    inputs['background'] = list(R.background(1, len(counts)))
    got = getattr(model, method)(inputs, labels)['seg'].cpu().numpy().astype(np.int64)
    ref = R.seg_from_overlay(fx[key + '_fg'], R.background(1, len(counts)).numpy(), key != 'seg_sem')
    assert got.shape == ref.shape
    assert set(np.unique(got).tolist()) == set(np.unique(ref).tolist())
    assert (got != ref).mean() <= 1e-4


# ------------------------------------------------------------------------------------------------- determinism and isolation
def _same(a, b):
    for k in OUTS:
        assert torch.equal(a[k], b[k]), k


def test_two_runs_are_bit_identical(model):
    args = _args(60, 9, 3, 3)
    _same(model(*args), model(*args))


def test_captured_forward_replays_bit_identical(model):
    args = _args(61, 12, 3, 3)
    eager = model(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model(*args)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = model(*args)
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    _same(cap, eager)
    assert model.fg_status() == 0


def test_instance_zero_alone_and_in_a_batch(model):
    args = _args(62, 37, 3, 3)
    full = model(*args)
    one = model(*[a[:1] if torch.is_tensor(a) else a for a in args])
    for k in OUTS:
        assert torch.equal(one[k][0], full[k][0]), k


def test_fp32_mode_is_untouched_by_a_pair_forward(model):
    """the caches keyed on the arithmetic do not leak: fp32, pair, fp32 on one model; the pair result differs from both"""
    args = _args(63, 5, 3, 3)
    with mode(model, 'fp32'):
        before = model(*args)
    pair = model(*args)
    with mode(model, 'fp32'):
        after = model(*args)
    _same(before, after)
    assert not torch.equal(pair['mask_feats'], before['mask_feats'])


# ----------------------------------------------------------------------------------------------------------------------- range
def _range_case(model, args, name, bit):
    from panoptic_forecasting_amd.lib import PfError
    with mode(model, 'fp32'):
        want = model(*args)
    with mode(model, on_range='raise'):
        with pytest.raises(PfError, match=name) as e:
            model(*args)
        assert ('status %d' % bit) in str(e.value)
    with mode(model, on_range='rerun'):
        _same(model(*args), want)
    with mode(model, on_range='ignore'):
        model(*args)
        assert model.fg_status() == bit
        assert model.fg_status() == 0


def test_overflow_is_flagged(model):
    args = _args(64, 3, 2, 2)
    args[3] = args[3].clone()
    args[3][1, 1, 200, 7, 7] = 1e5           # one staged value beyond 65504
    _range_case(model, args, r'PF_STATUS_RANGE \(', 1)


def test_tiny_features_are_flagged(model):
    args = _args(65, 3, 2, 2)
    args[3] = args[3] * 2.0 ** -20
    _range_case(model, args, 'PF_STATUS_RANGE_LOW', 2)


def test_all_zero_features_raise_nothing(model):
    args = _args(66, 3, 2, 2)
    args[3] = torch.zeros_like(args[3])
    model(*args)                              # fg_on_range = 'raise'
    assert model.fg_status() == 0


def test_status_after_captured_replays(model):
    args = _args(64, 3, 2, 2)
    args[3] = args[3].clone()
    args[3][1, 1, 200, 7, 7] = 1e5
    with mode(model, on_range='ignore'):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            model(*args)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert model.fg_status() == 1
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            model(*args)
        with mode(model, on_range='raise'):          # under capture nothing is read, whatever the mode
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                model(*args)
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        assert model.fg_status() == 1
        assert model.fg_status() == 0


# ---------------------------------------------------------------------------------------------------------------------- driver
def test_export_panoptic_takes_the_arithmetic_from_extra_args(tmp_path):
    """export_panoptic.main with --extra_args model.fg_arithmetic fp16_pair (nothing else added to the driver): its PNGs decode to what
    predict_panoptic of a pair model gives for the same batch - and the model the driver built was a pair model"""
    import yaml
    from PIL import Image
    import fgscene_tree as FT
    from oracle import panoptic as op
    from panoptic_forecasting_amd import export_panoptic, fg_dataset as D, fg_model, panoptic as pp
    from panoptic_forecasting_amd.registry import build_model
    scenes, data = FT.write_synthetic(str(tmp_path / 'data'), n_scenes=2, seed=5)
    config = {'task': 'fg', 'model': dict(R.FG_CONFIG, use_depth_sorting=True), 'data': data, 'training': {'batch_size': 2}}
    ckpt_dir = tmp_path / 'ckpt'
    ckpt_dir.mkdir()
    with open(str(ckpt_dir / 'config.yaml'), 'w') as f:
        yaml.safe_dump(config, f)
    params = R.fg_params(use_depth_sorting=True, fg_arithmetic='fp16_pair', fg_on_range='raise')
    params['no_gpu'] = False
    pair_model = build_model(params)
    pair_model.load_state_dict(R.fill_weights(pair_model.state_dict()))
    pair_model.save(str(ckpt_dir / 'fg_model.pt'))
    built = []
    init = fg_model.FGModel.__init__

    def spy(self, p):
        init(self, p)
        built.append(self)
    fg_model.FGModel.__init__ = spy
    try:
        out = export_panoptic.main(['--config_file', str(ckpt_dir / 'config.yaml'), '--load_model', str(ckpt_dir / 'fg_model.pt'),
                                    '--export_name', 'pan', '--working_dir', str(tmp_path / 'work'),
                                    '--extra_args', 'model.fg_arithmetic', 'fp16_pair', '--extra_args', 'model.fg_on_range', 'raise'])
    finally:
        fg_model.FGModel.__init__ = init
    assert [m.fg_arithmetic for m in built] == ['fp16_pair'] and built[0]._ws.get(1) is not None and built[0]._ws.get(0) is None
    result_dir, ann_file, n_ann = out[FT.SPLIT]
    ds = D.NativeFGSceneDataset(FT.SPLIT, {'data': dict(data)}, test=True)
    host = ds.host_batch(range(2))
    with torch.no_grad():
        seg = pair_model.predict_panoptic(host['inputs'], host['labels'])['seg']
    assert (seg >= 11000).any()
    names = sorted(os.listdir(os.path.join(result_dir, 'pan_val')))
    for b in range(2):
        ids = pp.decode_png(np.array(Image.open(os.path.join(result_dir, 'pan_val', names[b]))))
        _, want_ids, _ = op.encode(seg[b].cpu(), convert=True)
        assert np.array_equal(ids, want_ids), b
