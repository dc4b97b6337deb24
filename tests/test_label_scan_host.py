"""The [head | units | tail] split of an image by the count kernels of the semantic evaluators (csrc/label_scan.h: scan_span,
through pf_debug_label_scan_span): host code only, no GPU.  Every pair of base-pointer offsets, for the element sizes and
alignments conf_count_kernel and iiou_count_kernel instantiate, at image sizes around the unit sizes."""
import ctypes

import pytest

from panoptic_forecasting_amd import lib as pflib

BASE = 0x7f0000001000                       # 4096-aligned; the offsets below are added to it
SIZES = (0, 1, 3, 15, 16, 17, 31, 32, 33, 100)


def unit_align(esz, P):
    """bytes a lane's load of P elements of esz bytes must be aligned to: the load itself, 16 bytes at the most"""
    return min(P * esz, 16)


# (element size of map a, of map b, pixels of a unit): the prediction is u8 / i32 / i64, the other map u8 (confusion) or u16 (iIoU) /
# i32 / i64; a unit is 16 pixels where both maps are narrow, else 4
KINDS = [(1, 1, 16), (1, 2, 16)] + [(ea, eb, 4) for ea in (1, 4, 8) for eb in (1, 2, 4, 8) if (ea, eb) not in ((1, 1), (1, 2))]


def span(addr_a, addr_b, esz_a, esz_b, al_a, al_b, n, P):
    out = (ctypes.c_ulonglong * 5)()
    pflib.check(pflib.load().pf_debug_label_scan_span(addr_a, addr_b, esz_a, esz_b, al_a, al_b, n, P, out), 'pf_debug_label_scan_span')
    return tuple(out)


@pytest.mark.parametrize('esz_a,esz_b,P', KINDS)
def test_span_of_every_offset_pair(esz_a, esz_b, P):
    al_a, al_b = unit_align(esz_a, P), unit_align(esz_b, P)
    for off_a in range(0, 16, esz_a):
        for off_b in range(0, 16, esz_b):
            a, b = BASE + off_a, BASE + off_b
            both = [h for h in range(16) if (a + h * esz_a) % al_a == 0 and (b + h * esz_b) % al_b == 0]
            first = [h for h in range(16) if (a + h * esz_a) % al_a == 0]
            want = both[0] if both else first[0]
            for n in SIZES:
                head, units, tail0, ok_a, ok_b = span(a, b, esz_a, esz_b, al_a, al_b, n, P)
                where = (off_a, off_b, n)
                assert head == min(want, n), where                 # the fewest pixels aligning both maps, else the first; clamped
                assert head <= min(15, n), where
                assert tail0 == head + units * P and tail0 <= n < tail0 + P, where
                if n - head < P:
                    assert units == 0 and tail0 == head, where
                assert ok_a == ((a + head * esz_a) % al_a == 0) and ok_b == ((b + head * esz_b) % al_b == 0), where
                if both and n >= want:
                    assert ok_a and ok_b, where
                assert head + (n - tail0) < 32, where              # one 256-lane workgroup covers head and tail


def test_span_refuses_what_it_cannot_divide_by():
    L = pflib.load()
    out = (ctypes.c_ulonglong * 5)()
    assert L.pf_debug_label_scan_span(BASE, BASE, 1, 1, 16, 16, 100, 16, None) == -1
    for bad in ((0, 1, 16, 16, 16), (1, 0, 16, 16, 16), (1, 1, 0, 16, 16), (1, 1, 16, 0, 16), (1, 1, 16, 16, 0)):
        assert L.pf_debug_label_scan_span(BASE, BASE, bad[0], bad[1], bad[2], bad[3], 100, bad[4], out) == -1
        assert b'pf_debug_label_scan_span' in L.pf_last_error()
