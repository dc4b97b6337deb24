"""The store rule of the packed-pair layout (csrc/conv_epilogue.h: S4Dst, s4_store_px) per kernel that writes it: a slice of a shared
tensor that starts in the middle of a channel group (dst_choff % 4 == 2) next to slices that own half of their last group.

Block growth (10, 18) puts three slices of a 38-channel tensor at channels 0 / 10 / 20: the first starts on a group and owns half of group
2 (channels 8, 9), the second starts in the middle of that group and ends on a whole one, the third starts on a group and owns half of
group 9.  The writers that existing tests already run on these slices, against float64 at 2e-5 (1 + max |ref|) with the labels asserted:
  conv_s4_kernel, share + add       tests/test_gpu_share_s.py::test_share_add_vs_float64_and_two_launches (10, 18; its share_s = 0 run is
                                    the plain kernel), ::test_share_add_slices_that_start_in_the_middle_of_a_group (slices at 2 / 12 / 22)
  conv_pair_kernel, merged and not  tests/test_gpu_conv.py::test_conv_pair_vs_float64_and_two_launches (10, 18): P's slice at 10, C's at 20
  conv_s4_tail_kernel               tests/test_gpu_fold_final.py (10, 18, 5): stores fp32 only, the slices in front of its own bit for bit
  conv_s4_down_kernel<2 / 3>, lo    tests/test_gpu_fold_down.py (10, 18, 40) and (16, 20, 33) at 16 x 40 (the pooled packed tensor ends in
                                    half a group; at 10 x 36 it is fp32), tests/test_gpu_fold_wide.py (16, 46): the slice ends at 78.  The
                                    plan folds only a slice that starts on a group, and a pooled tensor is a tensor of its own
  conv_s4_1x1_kernel +pool / +res   tests/test_gpu_conv.py::test_packed_activation_block: pooled and residual outputs are tensors of their own
  conv_front                        tests/test_gpu_stem.py, tests/test_gpu_bg_model.py: its destination starts on a group (plan rule)
Writers whose packed store no schedule reaches:
  conv_s4_blocked_kernel            runs in the training step only, which sets dst_fmt = 0 for it (csrc/train_schedule.cpp: the layer's
                                    output goes to BatchNorm as fp32; tests/test_gpu_train.py runs it) - its packed branch is dead code
  conv_wave, conv_mfma              an fp32-source convolution writes packed pairs only where the schedule chose conv_dma or conv_split
                                    for it (csrc/hardnet_schedule.cpp: Step::can_write); the library has no entry point that launches
                                    one convolution, so their packed branch (the same epi_store) cannot be run from a test
  conv_split, conv_split1           chosen for an fp32-source convolution by the automatic rule only (forcing them turns the packed
                                    layout off: conv_mfma.h force_allows_s4); no case here makes the rule choose them
Left for this file, at 9 x 36 (one workgroup's tile with partial edges), B = 1: the plain 1x1 kernel, whose 16-byte pair store falls back to
the shared routine on exactly these slices; conv_dma through epi_store (stride-2 convs, and stride-1 convs over the fp32 network input)
writing such slices for a packed-pair reader; conv_dma through epi_store_pooled into a packed tensor that owns half of its last group."""
import pytest
import torch
import torch.nn.functional as F

from helpers import SLICES, pooled_net, slices_net
from test_gpu_fold_final import force_conv, run_labels  # noqa: F401

pytestmark = pytest.mark.gpu


def slices_ref(x, P, k, stride, src):
    D = {n: (v[0].double(), v[1].double()) for n, v in P.items()}
    t0 = F.relu(F.conv2d(x.double(), *D['t0'], padding=1)) if src == 't0' else x.double()
    ref = {n: F.relu(F.conv2d(t0, *D[n], padding=k // 2, stride=stride)) for n, _, _ in SLICES}
    ref['fin'] = F.conv2d(torch.cat([ref[n] for n, _, _ in SLICES], 1), *D['fin'], padding=1)
    return ref


# the label of A, B and C (t0 is conv_dma_kernel<3, 1, ..> in the first two cases; the third has no t0)
@pytest.mark.parametrize('k,stride,src,kernel', [(1, 1, 't0', 'conv_s4_1x1_kernel<'), (3, 2, 't0', 'conv_dma_kernel<3, 2,'),
                                                 (3, 1, 'input', 'conv_dma_kernel<3, 1,')],
                         ids=['s4_1x1', 'stride2_epi_store', 'fp32_input_epi_store'])
def test_slices_in_mid_group_and_half_owned_tails(k, stride, src, kernel, force_conv):
    """each slice of `out` against its own float64 reference after all three were written (in the order A, B, C: a writer that stored
    past its half of a group breaks the neighbour written before it)"""
    from helpers import MiniNet
    force_conv(5, 2, 0, 0)
    g = torch.Generator().manual_seed(17 * k + stride)
    h, w = 9 * stride, 36 * stride
    x = torch.randn(1, 12, h, w, generator=g) * torch.exp(0.5 * torch.randn(1, 12, 1, 1, generator=g))
    spec, P = slices_net(g, k, stride, src)
    ref = slices_ref(x, P, k, stride, src)
    net = MiniNet(spec, P)
    labels = run_labels(net, x)
    assert sum(kernel in l for l in labels) == 3, labels                               # A, B and C
    assert any('conv_s4_kernel' in l for l in labels), labels                          # fin reads `out` as packed pairs
    assert net.status() == 0
    out, fin = net.tensor('out').cpu(), net.tensor('fin').cpu()
    for name, off, ch in SLICES:
        r = ref[name].float()
        assert (out[:, off:off + ch] - r).abs().max().item() <= 2e-5 * (1.0 + r.abs().max().item()), name
    r = ref['fin'].float()
    assert (fin - r).abs().max().item() <= 2e-5 * (1.0 + r.abs().max().item())
    net.close()


def test_pooled_store_into_a_half_owned_last_group(force_conv):
    """dn (18 couts) + pool over the fp32 input at 18 x 72 -> 9 x 36 packed pairs: epi_store_pooled, channels 16, 17 own half of group 4"""
    from helpers import MiniNet
    force_conv(5, 2, 0, 0)
    g = torch.Generator().manual_seed(23)
    x = torch.randn(1, 12, 18, 72, generator=g) * torch.exp(0.5 * torch.randn(1, 12, 1, 1, generator=g))
    spec, P = pooled_net(g)
    D = {n: (v[0].double(), v[1].double()) for n, v in P.items()}
    pl = F.avg_pool2d(F.relu(F.conv2d(x.double(), *D['dn'])), 2)
    ref = {'pl': pl, 'fin': F.conv2d(pl, *D['fin'], padding=1)}
    net = MiniNet(spec, P)
    labels = run_labels(net, x)
    assert sum('conv_dma_kernel<1,' in l and '+pool' in l for l in labels) == 1, labels
    assert any('conv_s4_kernel' in l for l in labels), labels                          # fin reads `pl` as packed pairs
    assert net.status() == 0
    for name, r in ref.items():
        r = r.float()
        assert (net.tensor(name).cpu() - r).abs().max().item() <= 2e-5 * (1.0 + r.abs().max().item()), name
    net.close()
