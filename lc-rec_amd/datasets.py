"""Item-embedding input -- mirror of the reference's index/datasets.py (EmbDataset :6-21) plus the
device-resident loader the MI355X trainer iterates instead of a worker-process DataLoader.

Contract kept from the reference: `np.load` of an [N, d] float array (the `.emb-*-td.npy` written
by data_process/amazon_text_emb.py:101-105), `.dim`, `len()`, and `__getitem__` returning a
float32 tensor -- also for a LIST of indices (generate_indices.py:117 fancy-indexes collision
groups).
"""
import numpy as np
import torch
import torch.utils.data as data

_CAST_TORCH = {2: torch.float16, 8: torch.float64}       # element size -> staging dtype of to_device's "device" cast


class EmbDataset(data.Dataset):

    def __init__(self, data_path, mmap=False):
        self.data_path = data_path
        self.embeddings = np.load(data_path, mmap_mode="r" if mmap else None)
        self.dim = self.embeddings.shape[-1]
        self._device_copy = None

    def __getitem__(self, index):
        return torch.FloatTensor(np.asarray(self.embeddings[index]))

    def __len__(self):
        return len(self.embeddings)

    def _device_cast_refusal(self, device):
        """None when the file can be converted in HBM (lcrec_cast_rows), else what stands in the way."""
        e = self.embeddings
        if device.type != "cuda":
            return f"the target {device} is not a HIP device"
        if e.dtype.kind != "f" or e.dtype.itemsize not in _CAST_TORCH or not e.dtype.isnative:
            return f"the file's dtype {e.dtype.str} is not native-endian float16 or float64"
        if e.ndim != 2 or not e.flags.c_contiguous:
            return f"the file's array (shape {e.shape}) is not a C-contiguous [N, d] matrix"
        return None

    def casts_on_device(self, device):
        """Whether to_device(device) -- cast="auto" -- converts this file in HBM rather than in the host threads."""
        return self._device_cast_refusal(torch.device(device)) is None

    def to_device(self, device, chunk_rows=None, rows=None, workers=None, stages=None, cast="auto"):
        """The matrix (or the item range rows=(lo, hi), one rank's shard) as one fp32 tensor in HBM
        (Games: 16 859 x 4096 = 276 MB; a 288 GB MI355X holds 17 M such rows).  Cast and copied in row
        chunks so a large or memory-mapped file never needs a second full host copy.

        On a GPU the chunks (~32 MB) go through a ring of pinned staging buffers: `workers` host threads
        cast/copy chunks into them side by side (numpy releases the GIL for the copy; one thread moves
        ~10 GB/s out of the page cache, the link takes five times that), the calling thread queues the H2D
        copies in order on a side stream.  Measured: tools/ingest_probe.py, DESIGN.md section 5.

        cast: where a float16 / float64 file becomes fp32.  "host": in the worker threads (numpy), so the link carries
        fp32.  "device": the staging buffers hold the file's own dtype (the workers' copy is a memcpy), each chunk lands
        in a raw device buffer and ops.cast_rows converts it into its rows of the result on the side stream -- the same
        bits; ValueError for a file that is not native-endian C-contiguous float16 / float64, or a target that is not a
        HIP device.  "auto": "device" where it applies, else "host".  `cast` is checked before the kept copy of the whole
        matrix is looked up: an explicit "device" that does not apply raises even when a copy is already resident, and a
        resident copy is returned whichever path made it."""
        device = torch.device(device)
        if cast not in ("auto", "host", "device"):
            raise ValueError(f"cast must be 'auto', 'host' or 'device', got {cast!r}")
        refusal = None if cast == "host" else self._device_cast_refusal(device)
        if cast == "device" and refusal is not None:
            raise ValueError(f"EmbDataset.to_device(cast='device'): {refusal}")
        on_device = cast != "host" and refusal is None
        whole = rows is None
        if whole and self._device_copy is not None and self._device_copy.device == device:
            return self._device_copy
        first, last = (0, len(self)) if whole else (int(rows[0]), int(rows[1]))
        n = last - first
        out = torch.empty((n, self.dim), dtype=torch.float32, device=device)
        if chunk_rows is None:
            # ~32 MB of what the staging buffers hold; on the device path a multiple of 4 rows, so that every chunk's rows of
            # `out` start 16-byte aligned like its raw buffer does, whatever the width (the 16-byte form of lcrec_cast_rows)
            chunk_rows = max(1, (32 << 20) // ((self.embeddings.dtype.itemsize if on_device else 4) * max(self.dim, 1)))
            if on_device and chunk_rows > 4:
                chunk_rows -= chunk_rows % 4
        if device.type != "cuda":
            for lo in range(0, n, chunk_rows):
                hi = min(n, lo + chunk_rows)
                out[lo:hi].copy_(torch.from_numpy(np.ascontiguousarray(self.embeddings[first + lo:first + hi],
                                                                       dtype=np.float32)))
        elif n > 0:
            import concurrent.futures as cf
            import os
            step = min(chunk_rows, n)
            chunks = [(lo, min(n, lo + step)) for lo in range(0, n, step)]
            workers = max(1, min(workers or min(8, os.cpu_count() or 1), len(chunks)))
            ring = max(2, min(stages or 2 * workers, len(chunks)))
            staged = _CAST_TORCH[self.embeddings.dtype.itemsize] if on_device else torch.float32
            stage = [torch.empty((step, self.dim), dtype=staged, pin_memory=True) for _ in range(ring)]
            done = [torch.cuda.Event() for _ in range(ring)]
            copier = torch.cuda.Stream(device)
            raw = None
            if on_device:
                from . import ops
                # one raw device buffer per pinned slot, in the file's dtype; freed when this call returns (by then the side
                # stream has drained).  The side stream first lets the current one finish with whatever held this memory before.
                raw = [torch.empty((step, self.dim), dtype=staged, device=device) for _ in range(ring)]
                copier.wait_stream(torch.cuda.current_stream(device))
            src = self.embeddings

            def fill(i, wait):
                lo, hi = chunks[i]
                if wait:
                    done[i % ring].synchronize()         # the H2D copy that last read this buffer has finished
                np.copyto(stage[i % ring][:hi - lo].numpy(), src[first + lo:first + hi], casting="unsafe")

            try:
                with cf.ThreadPoolExecutor(max_workers=workers) as pool:
                    fills = {i: pool.submit(fill, i, False) for i in range(min(ring, len(chunks)))}
                    for i, (lo, hi) in enumerate(chunks):
                        fills.pop(i).result()
                        with torch.cuda.stream(copier):
                            if raw is None:
                                out[lo:hi].copy_(stage[i % ring][:hi - lo], non_blocking=True)
                            else:                        # (the event below then also covers the raw buffer's reuse)
                                raw[i % ring][:hi - lo].copy_(stage[i % ring][:hi - lo], non_blocking=True)
                                ops.cast_rows(raw[i % ring][:hi - lo], out=out[lo:hi])
                            done[i % ring].record(copier)
                        if i + ring < len(chunks):       # its buffer's event is recorded now: safe to hand to a worker
                            fills[i + ring] = pool.submit(fill, i + ring, True)
            finally:
                copier.synchronize()                     # (also on an error: no copy may still read a staging buffer when it is freed)
            torch.cuda.current_stream(device).wait_stream(copier)
        if whole:
            self._device_copy = out
        return out


class DeviceLoader:
    """Batches of a device-resident embedding matrix, with the reference DataLoader's semantics
    (index/main.py:86: shuffle=True, drop_last=False; generate_indices.py:77: shuffle=False).

    Shuffling reproduces torch's RandomSampler draw sequence from the global CPU generator -- one
    int64 for the loader iterator's base seed, one for the sampler seed, then
    torch.randperm(n, generator=Generator().manual_seed(seed)) -- so under `torch.manual_seed(s)`
    the batch composition is the one the reference's DataLoader yields.  No worker processes, no
    per-item Python: a batch is one index_select on the GPU.
    """

    def __init__(self, dataset, batch_size, shuffle, device, rank=0, world_size=1):
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self.device = torch.device(device)
        self.rank, self.world_size = rank, world_size
        self.data = dataset.to_device(self.device) if isinstance(dataset, EmbDataset) else dataset.to(self.device)

    def __len__(self):
        return (self.data.shape[0] + self.batch_size - 1) // self.batch_size

    def _check_same_seed(self, seed):
        """Data parallel: every rank must walk the same permutation (the global batches are cut from it).  The seeds come
        from each process's global CPU generator; anything that draws from it on one rank only would silently give that
        rank another order -- duplicated and missing items per global batch.  One tiny collective per epoch says so."""
        import torch.distributed as tdist
        if not tdist.is_initialized():
            return
        dev = self.device if tdist.get_backend() != "gloo" else "cpu"
        # int64 seeds as two exact doubles-free halves: MAX and MIN of (hi, lo) pairs must agree
        t = torch.tensor([seed, -seed], dtype=torch.int64, device=dev)
        tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
        if int(t[0]) != seed or int(t[1]) != -seed:
            raise RuntimeError("lcrec_amd.DeviceLoader: the ranks' shuffle seeds differ (something drew from torch's global "
                               "generator on one rank only); the epoch order would not be the single-process one")

    def __iter__(self):
        for lo, hi, order in self._walk():
            yield self.data[lo:hi] if order is None else self.data.index_select(0, order[lo:hi])

    def iter_selections(self):
        """The same walk as __iter__ without materialising the batches: (matrix, row-index vector) pairs -- the captured
        training step gathers straight into its input buffer (engine.TrainEngine.step_selected)."""
        for lo, hi, order in self._walk():
            if order is None:
                if getattr(self, "_arange", None) is None:
                    self._arange = torch.arange(self.data.shape[0], device=self.device)
                yield self.data, self._arange[lo:hi]
            else:
                yield self.data, order[lo:hi]

    def _walk(self):
        n = self.data.shape[0]
        if self.shuffle:
            torch.empty((), dtype=torch.int64).random_()                       # _BaseDataLoaderIter base seed
            seed = int(torch.empty((), dtype=torch.int64).random_().item())    # RandomSampler.__iter__
            if self.world_size > 1:
                self._check_same_seed(seed)
            g = torch.Generator()
            g.manual_seed(seed)
            order = torch.randperm(n, generator=g).to(self.device)
        else:
            order = None
        for lo in range(0, n, self.batch_size):
            hi = min(n, lo + self.batch_size)
            self.last_global_rows = hi - lo
            if self.world_size > 1:
                # item-sharded data parallel: every rank walks the same global batches and gathers only its own slice of each
                from .dist import batch_slice
                a, b = batch_slice(hi - lo, self.rank, self.world_size)
                lo, hi = lo + a, lo + b
            yield lo, hi, order
