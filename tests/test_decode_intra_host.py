"""Host: the two decode entries for intra blocks (svt_hip_decode_intra_device, svt_hip_decode_mixed_batch_device) exist at every layer -- exported
by the library, declared in include/svtvp9_hip.h, typed by binding.py -- and refuse a null context or workspace without touching a device.  The
arithmetic is checked on the GPU (tests/test_gpu_decode_intra.py)."""
import ctypes as C
import os
import re

import svt_testlib as T

B = T.B
ENTRIES = ("svt_hip_decode_intra_device", "svt_hip_decode_mixed_batch_device")


def test_both_symbols_are_exported_and_declared():
    lib = B.load()
    header = open(os.path.join(T.ROOT, "include", "svtvp9_hip.h")).read()
    for name in ENTRIES:
        assert name in B.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(\s*svt_hip_ctx\s*\*ctx,\s*svt_encdec_work\s*\*work,", header), name
    # the inter-only entry is still there, with the signature the mixed one shares
    one = re.search(r"int32_t svt_hip_decode_batch_device\((.*?)\);", header, re.S).group(1)
    two = re.search(r"int32_t svt_hip_decode_mixed_batch_device\((.*?)\);", header, re.S).group(1)
    assert re.sub(r"\s+", " ", one) == re.sub(r"\s+", " ", two)


def test_binding_gives_them_argtypes():
    lib = B.load()
    vp, i32 = C.c_void_p, C.c_int32
    # (ctx, work, pic, width, height, mi_stride, q_index, thr, pad_x, pad_y, d_status)
    assert list(lib.svt_hip_decode_intra_device.argtypes) == [vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp]
    # (ctx, work, n_pics, pics, width, height, mi_stride, q_index, thr, pad_x, pad_y, d_status)
    assert list(lib.svt_hip_decode_mixed_batch_device.argtypes) == [vp, vp, i32, vp, i32, i32, i32, i32, vp, i32, i32, vp]
    assert list(lib.svt_hip_decode_mixed_batch_device.argtypes) == list(lib.svt_hip_decode_batch_device.argtypes)


def test_null_context_or_workspace_is_a_bad_parameter():
    """answered from the argument checks alone: no context exists in this process, so nothing can have been enqueued"""
    lib = B.load()
    pic, status, thr = B.EncdecPicture(), (C.c_int32 * 4)(7, 7, 7, 7), B.LfThresh()
    fake = C.c_void_p(0x1000)                                       # never dereferenced: the null argument is found first
    for ctx, work in ((None, fake), (fake, None), (None, None)):
        assert lib.svt_hip_decode_intra_device(ctx, work, C.byref(pic), 64, 64, 8, 100, C.byref(thr), 80, 80, status) == B.ERR_BAD_PARAMETER
        assert b"decode_intra" in lib.svt_hip_last_error()
        assert lib.svt_hip_decode_mixed_batch_device(ctx, work, 1, C.byref(pic), 64, 64, 8, 100, C.byref(thr), 80, 80, status) == B.ERR_BAD_PARAMETER
        assert b"decode" in lib.svt_hip_last_error()
    assert list(status) == [7, 7, 7, 7]
