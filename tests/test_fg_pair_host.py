"""The fg forecaster's fp16-pair option (PF_FG_PAIR, model.fg_arithmetic = 'fp16_pair'), host side (no GPU): the ABI's flag
handling and sizes, the model keys, and a float64 emulation of the pair GEMM that pins the term tests/test_gpu_fg_pair.py adds to
its derived bars and the weight scale rule of pf_fg_pack."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fg_ref64 as R
from panoptic_forecasting_amd import lib as pflib
from panoptic_forecasting_amd.fg_model import FGModel

PF_FG_PAIR = 1
PF_EUNSUPPORTED = -5
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pfhip.h')


def test_abi_accepts_the_pair_flag_and_nothing_else():
    L = pflib.load()
    raw0, packed0, raw1, packed1 = (ctypes.c_size_t() for _ in range(4))
    assert L.pf_fg_weights_size(0, ctypes.byref(raw0), ctypes.byref(packed0)) == 0
    assert L.pf_fg_weights_size(PF_FG_PAIR, ctypes.byref(raw1), ctypes.byref(packed1)) == 0
    assert raw1.value == raw0.value
    assert packed1.value >= packed0.value
    for flags in (2, 3):
        assert L.pf_fg_weights_size(flags, ctypes.byref(raw1), ctypes.byref(packed1)) == PF_EUNSUPPORTED
        assert b'flags' in L.pf_last_error()
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r'^#define\s+PF_FG_PAIR\s+1\s*$', text, re.M)
    for name in ('pf_fg_status', 'pf_fg_status_reset', 'pf_fg_pair_workspace'):
        assert re.search(r'^int %s\(' % name, text, re.M)
    # the workspace of the pair path = the flags = 0 workspace behind the status block; its size comes from a call of its own,
    # pf_fg_workspace goes on refusing every non-zero flags value (tests/test_fg_host.py)
    ws0, ws1 = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.pf_fg_workspace(5, 3, 3, 0, ctypes.byref(ws0)) == 0 and L.pf_fg_pair_workspace(5, 3, 3, ctypes.byref(ws1)) == 0
    assert L.pf_fg_workspace(5, 3, 3, PF_FG_PAIR, ctypes.byref(ws1)) == PF_EUNSUPPORTED
    assert L.pf_fg_pair_workspace(5, 3, 17, ctypes.byref(ws0)) == -1 and L.pf_fg_pair_workspace(0, 3, 3, ctypes.byref(ws0)) == 0
    assert L.pf_fg_workspace(5, 3, 3, 0, ctypes.byref(ws0)) == 0
    status_bytes = int(re.search(r'^#define\s+PF_FG_STATUS_BYTES\s+(\d+)', text, re.M).group(1))
    assert ws1.value == ws0.value + status_bytes
    assert L.pf_fg_workspace(5, 3, 3, 3, ctypes.byref(ws1)) == PF_EUNSUPPORTED
    # argument checks come before any device work under the flag too
    assert L.pf_fg_forward(None, PF_FG_PAIR, 0, 3, 3, 6, *([None] * 14), None, 0, None) == 0      # N = 0: nothing enqueued
    assert L.pf_fg_forward(None, PF_FG_PAIR, 4, 3, 3, 5, *([None] * 14), None, 0, None) == -1
    assert L.pf_fg_forward(None, 2, 0, 3, 3, 6, *([None] * 14), None, 0, None) == PF_EUNSUPPORTED


def test_model_keys():
    assert FGModel(R.fg_params()).fg_arithmetic == 'fp32'
    assert FGModel(R.fg_params(fg_arithmetic='fp32')).fg_arithmetic == 'fp32'
    m = FGModel(R.fg_params(fg_arithmetic='fp16_pair'))
    assert m.fg_arithmetic == 'fp16_pair' and m.fg_on_range == 'rerun' and m.fg_status() == 0
    with pytest.raises(ValueError, match='fg_arithmetic'):
        FGModel(R.fg_params(fg_arithmetic='bf16'))
    for v in ('rerun', 'raise', 'ignore'):
        assert FGModel(R.fg_params(fg_arithmetic='fp16_pair', fg_on_range=v)).fg_on_range == v
    with pytest.raises(ValueError, match='fg_on_range'):
        FGModel(R.fg_params(fg_on_range='clamp'))


def test_extra_args_reach_the_model(tmp_path):
    """what export_panoptic.py needs: --extra_args model.fg_arithmetic fp16_pair through the existing config path"""
    import yaml
    from panoptic_forecasting_amd.config import load_config
    cfg = tmp_path / 'config.yaml'
    p = R.fg_params()
    cfg.write_text(yaml.safe_dump({'task': 'fg', 'model': p['model'], 'data': {'odom_size': R.ODOM}}))
    got = load_config(argv=['--working_dir', str(tmp_path), '--config_file', str(cfg), '--extra_args', 'model.fg_arithmetic', 'fp16_pair',
                            '--extra_args', 'model.fg_on_range', 'raise'])
    assert got['model']['fg_arithmetic'] == 'fp16_pair' and got['model']['rnn_type'] == 'gru'
    m = FGModel(got)
    assert m.fg_arithmetic == 'fp16_pair' and m.fg_on_range == 'raise'


# ------------------------------------------------------------------------------------------------- the pair GEMM in float64
def scale_exponent(w):
    """k of pf_fg_pack: max |w * 2^k| in [2^14, 2^15); 0 for an all-zero tensor"""
    m = float(np.abs(np.asarray(w, dtype=np.float64)).max())
    if m == 0.0:
        return 0
    return 14 - (np.frexp(m)[1] - 1)


def split(x):
    """hi = fp16_rne(x), mid = fp16_rne(x - hi) of an fp32 tensor (x - hi is exact in fp32), both as float64"""
    x = x.float()
    hi = x.half()
    mid = (x - hi.float()).half()
    return hi.double(), mid.double()


@pytest.mark.parametrize('w,lo', [(np.array([0.0361, -0.02]), None), (np.array([1.0]), 2.0 ** 14), (np.array([3e-30, 1e-31]), None),
                                  (np.array([65504.0 * 4]), None), (np.array([2.0 ** -15 * 1.9999]), None)])
def test_scale_rule(w, lo):
    k = scale_exponent(w)
    top = float(np.abs(w).max()) * 2.0 ** k
    assert 2.0 ** 14 <= top < 2.0 ** 15
    if lo is not None:
        assert top == lo


def test_scale_rule_of_zeros():
    assert scale_exponent(np.zeros(7)) == 0


def test_pair_gemm_stays_within_the_derived_term():
    """The first cell's GEMM (h = 0: K = 272 * 9) on the generator's weights and inputs, 64 gate rows x one instance: both operands
    split as the kernel splits them, the three products hi*hi + hi*mid + mid*hi formed and summed in float64 (a product of two fp16
    numbers is exact there).  What is left is the operand error 2^-23 per operand and the dropped mid*mid <= 2^-22, together
    2^-21 sum |a| |w|: the term the GPU tests add to (2K + 2) 2^-24."""
    shape = (1024, 528, 3, 3)
    stream = list(FGModel(R.fg_params()).state_dict().keys()).index('mask_encoder.cell_list.0.conv.weight')
    rows = 64
    a = (3.0 / (528 * 9)) ** 0.5
    w = R.sym(stream, shape, a)[:rows, :272].contiguous()       # fill_weights' tensor for this key (stream = its state_dict index)
    inputs, _ = R.make_inputs(38, [1], t_in=1, t_out=1)
    feats = inputs['feats'][0][:, 0]                            # [1, 256, 14, 14]
    vec = R.sym(7, (1, 16), 2.0)[:, :, None, None].expand(-1, -1, 14, 14)
    x = torch.cat([vec, feats], 1).float()
    exact = F.conv2d(x.double(), w.double(), padding=1)
    k = scale_exponent(w.numpy())
    ws = torch.ldexp(w, torch.tensor(k))
    assert 2.0 ** 14 <= float(ws.abs().max()) < 2.0 ** 15 and torch.equal(torch.ldexp(ws, torch.tensor(-k)), w)
    xh, xm = split(x)
    wh, wm = split(ws)
    conv = lambda p, q: F.conv2d(p, q, padding=1)
    pair = (conv(xh, wh) + conv(xh, wm) + conv(xm, wh)) * 2.0 ** -k
    bound = 2.0 ** -21 * conv(x.double().abs(), w.double().abs())
    ratio = float(((pair - exact).abs() / bound).max())
    print('pair GEMM, K = %d: worst |pair - exact| / (2^-21 sum|a||w|) = %.4g' % (272 * 9, ratio))
    assert ratio <= 1.0
    assert float((pair - exact).abs().max()) > 0                # the emulation does differ from the exact sum
    # the operand bound itself, on these operands: |x - hi - mid| <= 2^-23 |x| + 2^-25
    for v, (h, m) in ((x, (xh, xm)), (ws, (wh, wm))):
        assert bool(((v.double() - h - m).abs() <= 2.0 ** -23 * v.double().abs() + 2.0 ** -25).all())
