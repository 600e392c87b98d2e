"""HIP-graph replay of the launch-bound, sync-free parts of a step (feature path, aggregation).

``GraphedCall(fn)`` runs ``fn(tensors)`` once per input signature under stream capture (torch.cuda.CUDAGraph drives
hipStreamBeginCapture / hipGraphInstantiate; every kernel of this package is launched on torch's current stream, so the
ctypes launches are captured like torch's own) and afterwards replays the ~300 launches with ONE hipGraphLaunch: the CPU cost
of the feature path drops from ~3 ms of Python/ctypes per batch to ~0.1 ms, the device work is the same kernels in the same
order (bit-identical outputs).  Inputs are copied into buffers owned by the graph; outputs are the graph's own tensors and are
overwritten by the next replay of the same entry -- callers clone what must outlive the step.
"""
import gc
import threading

import torch

_CAPTURE_LOCK = threading.Lock()


class GraphedCall:
    def __init__(self, fn, device, max_entries=4):
        self.fn, self.dev, self.entries, self.max_entries = fn, device, {}, max_entries
        self.disabled = False

    def __call__(self, tensors, extra_key=()):
        if self.disabled:
            return self.fn(tensors)
        key = tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(tensors.items())) + tuple(extra_key)
        e = self.entries.get(key)
        if e is None:
            while len(self.entries) >= self.max_entries:            # each entry owns a private memory pool: bound them
                self.entries.pop(next(iter(self.entries)))
            try:
                e = self._capture(tensors)
            except (RuntimeError, torch.AcceleratorError) as err:   # capture refused (e.g. a foreign thread touched the device):
                from ..ops import VphoError                         # same kernels, launched one by one from here on
                if isinstance(err, VphoError):
                    raise
                import warnings
                warnings.warn(f'HIP graph capture failed ({err}); falling back to plain launches for this call site')
                self.disabled = True
                return self.fn(tensors)
            self.entries[key] = e
        static, graph, out = e
        dev_in = [k for k, v in tensors.items() if v.is_cuda]
        if len(dev_in) > 1:                                   # one multi-tensor copy instead of a launch per input
            torch._foreach_copy_([static[k] for k in dev_in], [tensors[k] for k in dev_in], non_blocking=True)
        else:
            dev_in = []
        for k, v in tensors.items():
            if k not in set(dev_in):
                static[k].copy_(v, non_blocking=True)
        graph.replay()
        return out

    def _capture(self, tensors):
        # One capture at a time, and no device-wide synchronisation in here: hipDeviceSynchronize from any thread is an
        # error while another thread's stream is capturing (stream-level waits are fine).
        with _CAPTURE_LOCK:
            static = {k: v.detach().clone() for k, v in tensors.items()}
            cur = torch.cuda.current_stream(self.dev)
            side = torch.cuda.Stream(self.dev)
            side.wait_stream(cur)
            with torch.cuda.stream(side):                  # eager pass: one-time attribute opt-ins, allocator warm-up
                self.fn(static)
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            # No garbage collection while the stream captures: a dead reference cycle that owns device memory (an earlier GraphedCall's
            # graph and its pool) would be freed in the middle of the capture, which the runtime refuses -- from a destructor, so the
            # process aborts.  torch.cuda.graph used to collect on entry; since it stopped, when a collection falls is a matter of
            # how many objects the launches in between happen to allocate.
            gc.collect()
            collecting = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(graph, stream=side, capture_error_mode='thread_local'):
                    out = self.fn(static)
            finally:
                if collecting:
                    gc.enable()
            cur.wait_stream(side)
        return static, graph, out
