"""`--sampler reference` of the CLIs: the reference's own batches, drawn by native host code (macr_ref_sample_batches).

The batches of MFData.sample, LGCNData.sample and LGCNData.sample_test (macr_mf/load_data.py:543-566,
macr_lightgcn/utility/load_data.py:174-212, :214-254 of the reference) are a function of the `random` and `numpy.random`
generator states.  This sampler reads those LIVE states at the start of a pass, draws the whole pass in C++, and writes the
states the Python loops would have left back into the modules, Gaussian-cache fields included.  Between passes nothing can
tell the two forms apart: `train_state` checkpoints and `--resume 1` are interchangeable, a Python-form pass may follow a
native one, and anything else that draws from those modules sees the same numbers.

Same `.sample()` -> (3,B) int32 tensor contract as sampler.DeviceSampler, plus `begin_pass(n)` before the first batch of a
pass.  Generation is synchronous, once per pass; no worker thread, nothing is drawn ahead of the pass that needs it.
"""
import ctypes
import random
import time

import numpy as np
import torch

from . import _lib

PINNED_CHUNK_BYTES = 8 << 20          # staging per upload (two such buffers alternate); a pass itself may be ~100 MB


def _csr(rows, what):
    """(ptr int32[n+1], idx int32[nnz]) of a list of lists, entries in the order given"""
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    if ptr[-1] >= 2 ** 31:
        raise ValueError("%s: %d entries do not fit int32 offsets" % (what, ptr[-1]))
    idx = np.fromiter((x for r in rows for x in r), dtype=np.int32, count=int(ptr[-1]))
    if idx.size == 0:
        idx = np.zeros(1, dtype=np.int32)          # (a valid pointer for an all-empty table)
    return ptr.astype(np.int32), idx


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


class ReferenceStreamSampler(object):
    def __init__(self, kind, population, pos_lists, excl_lists, n_users, n_items, batch_size, device=None,
                 chunk_batches=None):
        """kind: _lib.REFSTREAM_MF | REFSTREAM_LGCN.  population: user ids in the order the reference's list has them.
        pos_lists / excl_lists: one list per user id 0..n_users-1 -- positives in LIST order (a draw is an index into
        the list), exclusions in any order (stored ascending, de-duplicated).  device=None: sample() returns host tensors.
        chunk_batches: batches per native call and per upload (default: what fits PINNED_CHUNK_BYTES); the batches and
        the states do not depend on it."""
        self.kind, self.n_users, self.n_items, self.batch_size = int(kind), int(n_users), int(n_items), int(batch_size)
        self.pop = np.ascontiguousarray(np.asarray(list(population), dtype=np.int32))
        self.pos_ptr, self.pos_idx = _csr(pos_lists, "positives")
        self.excl_ptr, self.excl_idx = _csr([sorted(set(r)) for r in excl_lists], "exclusions")
        self.device = None if device is None else torch.device(device)
        if chunk_batches is None:
            chunk_batches = PINNED_CHUNK_BYTES // (12 * max(self.batch_size, 1))
        self.chunk_batches = max(1, int(chunk_batches))
        self._ws = np.empty(max(1, _lib.lib().macr_ref_sample_workspace_bytes(len(self.pop))), dtype=np.uint8)
        self._host = self._dev = self._pinned = None
        self._n = self._k = 0
        self.passes, self.seconds_in_begin_pass = 0, 0.0      # what tools/bench_reference_sampler.py and the CLIs report

    @classmethod
    def for_mf(cls, data, device=None, batch_size=None, chunk_batches=None):
        """the stream of MFData.sample (macr_mf/load_data.py:543-566): population range(n_users), positives and
        exclusions the train lists"""
        train = [data.train_user_list.get(u, ()) for u in range(data.n_users)]
        return cls(_lib.REFSTREAM_MF, range(data.n_users), train, train, data.n_users, data.n_items,
                   data.batch_size if batch_size is None else batch_size, device, chunk_batches)

    @classmethod
    def for_lgcn(cls, data_generator, test=False, device=None, batch_size=None, chunk_batches=None):
        """the stream of LGCNData.sample (utility/load_data.py:174-212: population exist_users, positives and exclusions
        the train lists) or, test=True, of sample_test (:214-254: population the keys of test_set, positives the test
        lists, exclusions test and train lists together)"""
        dg = data_generator
        train = [dg.train_items.get(u, ()) for u in range(dg.n_users)]
        if not test:
            pop, pos, excl = dg.exist_users, train, train
        else:
            pop = list(dg.test_set.keys())
            pos = [dg.test_set.get(u, ()) for u in range(dg.n_users)]
            excl = [list(p) + list(t) for p, t in zip(pos, train)]
        return cls(_lib.REFSTREAM_LGCN, pop, pos, excl, dg.n_users, dg.n_items,
                   dg.batch_size if batch_size is None else batch_size, device, chunk_batches)

    def generate(self, n, out=None):
        """n batches from the live `random` / `numpy.random` states into a (n,3,B) int32 numpy array; the states the Python
        form would have left are written back into the modules.  A refusal (macr_amd._lib.MacrError) changes nothing."""
        B = self.batch_size
        if out is None:
            out = np.empty((n, 3, B), dtype=np.int32)
        ver, internal, gauss = random.getstate()
        np_kind, np_keys, np_pos, has_gauss, cached = np.random.get_state()
        py_key = np.array(internal[:624], dtype=np.uint32)
        py_pos = ctypes.c_int(internal[624])
        np_key = np.array(np_keys, dtype=np.uint32)
        np_pos = ctypes.c_int(int(np_pos))
        L = _lib.lib()
        for lo in range(0, n, self.chunk_batches):
            m = min(self.chunk_batches, n - lo)
            _lib.check(L.macr_ref_sample_batches(
                self.kind, m, B, self.n_users, _p(self.pop), len(self.pop), _p(self.pos_ptr), _p(self.pos_idx),
                _p(self.excl_ptr), _p(self.excl_idx), self.n_items, _p(py_key), ctypes.byref(py_pos), _p(np_key),
                ctypes.byref(np_pos), ctypes.c_void_p(out.ctypes.data + lo * 12 * B), _p(self._ws), self._ws.nbytes))
        random.setstate((ver, tuple(py_key.tolist()) + (py_pos.value,), gauss))
        np.random.set_state((np_kind, np_key, np_pos.value, has_gauss, cached))
        return out

    def begin_pass(self, n):
        """Draw the n batches of the coming pass (the live states move on by exactly that pass) and start their upload:
        chunk by chunk through two alternating pinned buffers, one non-blocking copy each."""
        t0 = time.perf_counter()
        B = self.batch_size
        if self._host is None or self._host.shape[0] < n:
            self._host = np.empty((n, 3, B), dtype=np.int32)
        self.generate(n, self._host)
        if self.device is not None:
            if self._dev is None or self._dev.shape[0] < n:
                self._dev = torch.empty((n, 3, B), dtype=torch.int32, device=self.device)
            if self._pinned is None:
                rows = min(self.chunk_batches, max(n, 1))
                self._pinned = [[torch.empty((rows, 3, B), dtype=torch.int32).pin_memory(), None] for _ in range(2)]
            host = torch.from_numpy(self._host)
            rows = self._pinned[0][0].shape[0]
            for k, lo in enumerate(range(0, n, rows)):
                m = min(rows, n - lo)
                slot = self._pinned[k & 1]
                if slot[1] is not None:
                    slot[1].synchronize()              # the upload that last read this buffer
                slot[0][:m].copy_(host[lo:lo + m])
                self._dev[lo:lo + m].copy_(slot[0][:m], non_blocking=True)
                slot[1] = torch.cuda.Event()
                slot[1].record()
        self._n, self._k = n, 0
        self.passes += 1
        self.seconds_in_begin_pass += time.perf_counter() - t0

    def sample(self):
        """-> the next (3,B) int32 batch of the pass: a view of the pass's buffer (device tensor, or host tensor with
        device=None), valid until the next begin_pass.  It carries its host view as `_macr_host_batch`, as
        mf.ShardedBPRMF.to_device_batch does: the routing of the row-sharded step then needs no device read."""
        if self._k >= self._n:
            raise RuntimeError("ReferenceStreamSampler.sample: batch %d of a pass of %d (begin_pass(n) draws a pass)"
                               % (self._k, self._n))
        hv = self._host[self._k]
        batch = torch.from_numpy(hv) if self.device is None else self._dev[self._k]
        batch._macr_host_batch = hv
        self._k += 1
        return batch
