"""Ties the host-side dump of the inference schedule (pf_debug_hardnet_schedule, tests/test_hardnet_schedule_host.py) to what a forward
launches: the convolution kernels named by the profile labels of one forward are the ones the debug rows name."""
import pytest
import torch

from test_gpu_fold_final import force_conv, run_labels  # noqa: F401
from test_gpu_fold_wide import all_forms_net
from test_hardnet_schedule_host import CI, KIND, KIND_NAME, KS, NO_BIAS, NT, POOL, RES, TH, TW, folds, mini  # noqa: F401
from test_share_s_host import option  # noqa: F401

pytestmark = pytest.mark.gpu

S4_FORM = {'S_CONV_S4_SHARE': 'conv_s4_share_kernel', 'S_CONV_S4_ADD': 'conv_s4_add_kernel', 'S_CONV_S4_TAIL': 'conv_s4_tail_kernel',
           'S_CONV_S4_DOWN': 'conv_s4_down_kernel', 'S_CONV_S4_LO': 'conv_s4_lo_kernel'}
# the fp32-source kernels carry template arguments the rows do not hold (epilogue, wave counts): compared by family
FAMILY = {'S_CONV_GENERIC': 'conv_mfma_kernel', 'S_CONV_SPLIT': 'conv_split_kernel', 'S_CONV_SPLIT1': 'conv_split1_kernel',
          'S_CONV_WAVE': 'conv_wave_kernel', 'S_CONV_DMA': 'conv_dma_kernel', 'S_PAIR': 'conv_pair_kernel'}


def kernel_of(spec, r):
    """the profile label of a convolution step's launch (csrc/conv_s4.hip: launch_s4_form; conv_s4_1x1.hip: launch_s41_cfg), or its kernel family"""
    kind = KIND_NAME[r[KIND]]
    if kind in FAMILY:
        return FAMILY[kind]
    if kind == 'S_CONV_S4' and spec.ops[r[CI]].k == 1:
        fused = r[POOL] or r[RES] or r[NO_BIAS]
        return ('void pf::conv_s4_1x1_kernel<%d, %d>(pf::ConvArgs)' % (r[NT], int(bool(fused))) + (' +res' if r[RES] else '') +
                (' +pool' if r[POOL] else '') + (' lowres-half' if r[NO_BIAS] else ''))
    return 'void pf::%s<%d, %d, %d, %d>(pf::ConvArgs)' % (S4_FORM.get(kind, 'conv_s4_kernel'), r[NT], r[TW], r[TH], r[KS])


def test_profile_labels_of_a_forward_name_the_kernels_of_the_debug_rows(folds, force_conv):  # noqa: F811
    from helpers import MiniNet
    force_conv(5, 3, 0, 0)
    folds(2)                                                          # process-wide: the plan below is created with them too
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, 12, 16, 64, generator=g)
    spec, P = all_forms_net(g)
    _, _, rows = mini((spec, P), 1, 16, 64)
    want = sorted(kernel_of(spec, r) for r in rows.tolist() if r[CI] >= 0)
    net = MiniNet(spec, P)
    labels = [l for l in run_labels(net, x) if 'conv_' in l]
    assert net.status() == 0
    net.close()
    got = sorted(l if 'conv_s4' in l else l.split('pf::')[1].split('<')[0] for l in labels)
    assert got == want
    assert sum('tail' in l or 'down' in l or '_lo_' in l for l in got) == 4 and any('lowres' not in l and '+res' in l for l in got)
