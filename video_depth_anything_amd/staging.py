"""What the "numpy in, bytes out" paths share (deflate, exr, mjpeg, visualize, scale): which device a call runs on,
how many frames fit a staging budget, and the block-by-block upload of a host array or memory map through one pinned block.
Uploads only, one block in flight: lanes.HostCopyRing and pointcloud.write_pointclouds own the overlapped downloads."""
import numpy as np


def cuda_device(device, who, twin=None):
    """torch.device(device), "cuda" for None; anything but a cuda device is an error that names the host twin."""
    import torch
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError(f"{who}: needs a cuda device, got {device!r}" + (f"; {twin} is the host twin" if twin else ""))
    return dev


def placement(data, device, who, twin, fn=None):
    """(is_tensor, device): a cuda tensor is used in place on its device, anything but a tensor goes to `device`; a host tensor is
    an error. `fn`: the function the error names behind `who`."""
    import torch
    if not isinstance(data, torch.Tensor):
        return False, cuda_device(device, who, twin)
    if not data.is_cuda:
        raise ValueError(f"{who}: {fn + ' ' if fn else ''}takes a cuda tensor or a numpy array; {twin} is the host twin")
    return True, data.device


def one_device(tensors, device, what):
    """The device the CUDA tensors among `tensors` (None entries skipped) share, or torch.device(device) when none is on a device."""
    import torch

    on_dev = [t.device for t in tensors if t is not None and t.is_cuda]
    dev = on_dev[0] if on_dev else torch.device(device)
    if dev.type != "cuda" or any(d != dev for d in on_dev):
        raise ValueError(f"{what}: needs one cuda device, got {device!r} / {[str(d) for d in on_dev]}")
    return dev


def frames_per_block(n, frame_bytes, budget):
    """How many of n frames are staged at a time: what fits the budget, at least one."""
    return max(1, min(n, budget // frame_bytes))


class Staged:
    """A pinned host block of `cap` items of `item_shape` and `dtype` (`host`) and its twin on `device` (`dev`), allocated once."""

    def __init__(self, cap, item_shape, dtype, device="cuda"):
        import torch
        self.cap = int(cap)
        self.host = torch.empty((self.cap,) + tuple(item_shape), dtype=dtype).pin_memory()
        self.dev = torch.empty_like(self.host, device=device)
        self._uploaded = torch.cuda.Event()

    def blocks(self, src, casting="no"):
        """(lo, m, dev[:m]) for consecutive runs of at most `cap` items of src (an ndarray or a memory map, read a run at a time),
        each uploaded on the device's current stream. The host block is written again only once its last upload has finished,
        whatever the consumer does with the view; the view itself holds until the next run is asked for."""
        import torch
        host = self.host.numpy()
        for lo in range(0, src.shape[0], self.cap):
            m = min(self.cap, src.shape[0] - lo)
            self._uploaded.synchronize()                                    # (an event never recorded does not wait)
            np.copyto(host[:m], src[lo:lo + m], casting=casting)
            self.dev[:m].copy_(self.host[:m], non_blocking=True)
            self._uploaded.record(torch.cuda.current_stream(self.dev.device))
            yield lo, m, self.dev[:m]
