"""What the kernel tests of the text tables share to hand device buffers to libs2c's C ABI
(imported like batch_model; torch is imported on use, so collecting needs no GPU)."""
import ctypes as C

import numpy as np


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_i64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64).reshape(-1)).cuda()
