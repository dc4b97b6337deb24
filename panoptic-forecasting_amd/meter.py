"""What the device meters (pq.PanopticQuality, semantic_iou.SemanticIoU) and gt_prep.GTPreparer share: workspaces that begin with a
sticky status word.

A workspace ``which`` belongs to the entry points pf_<which>_workspace / _accumulate / _status / _status_reset of include/pfhip.h:
bytes [0, 256) hold the status word and are cleared by the host only, everything behind them is zeroed by every call.
"""
import ctypes

import torch


class DeviceMeter:
    WORKSPACES = {}      # which -> (attribute that holds its tensor, how the growth error names it: '' or 'name ')
    HOST_PATH = ''       # the function that does the same on the host, for the refusal of a CPU device
    ENQUEUE = 'update'   # the method that enqueues a call, for the growth error

    def __init__(self, device):
        from . import lib as _lib
        self._lib = _lib
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.PfError('%s runs on the GPU (got %s): use %s on the host' % (type(self).__name__, self.device, self.HOST_PATH))
        for attr, _ in self.WORKSPACES.values():
            setattr(self, attr, None)
        self._captured = False

    def _call(self, which, what, *args):
        name = 'pf_%s_%s' % (which, what)
        self._lib.check(getattr(self._lib.load(), name)(*args), name)

    def _workspace(self, b, which):
        """The workspace grows with the largest B seen.  A captured graph keeps the pointer it was captured with, so a
        workspace may not grow during a capture or after one: call the enqueuing method once with the largest batch before capturing."""
        attr, label = self.WORKSPACES[which]
        old = getattr(self, attr)
        need = ctypes.c_size_t()
        self._call(which, 'workspace', b, ctypes.byref(need))
        capturing = torch.cuda.is_current_stream_capturing()
        if old is None or old.numel() < need.value:
            if capturing or self._captured:
                raise self._lib.PfError('%s: the %sworkspace would have to grow to B = %d %s a graph capture, whose replays '
                                        'keep the old pointer: call %s() with the largest batch before capturing'
                                        % (type(self).__name__, label, b, 'during' if capturing else 'after', self.ENQUEUE))
            ws = torch.zeros(need.value, dtype=torch.uint8, device=self.device)    # status word starts at 0
            if old is not None:
                ws[:256].copy_(old[:256])                                            # a sticky bit survives the growth
            setattr(self, attr, ws)
        self._captured = self._captured or capturing
        return getattr(self, attr)

    def _status_word(self, which):
        """The sticky status word of one workspace, 0 while it does not exist (waits for the current stream)."""
        ws = getattr(self, self.WORKSPACES[which][0])
        st = ctypes.c_int()
        if ws is not None:
            self._call(which, 'status', ws.data_ptr(), self._lib.stream_ptr(), ctypes.byref(st))
        return st.value

    def _status_reset(self):
        for which, (attr, _) in self.WORKSPACES.items():
            ws = getattr(self, attr)
            if ws is not None:
                self._call(which, 'status_reset', ws.data_ptr(), self._lib.stream_ptr())
