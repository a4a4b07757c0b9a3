"""Shared by the tests of the entropy pass's coefficient-update mode (test_entropy_coef_host.py, test_gpu_entropy_coef.py): the host form
svt_hip_entropy_picture_coef behind entropy_model.host_entropy's interface, the four real-stream pictures of
tests/golden/coef_update_reference.npz as the entry takes them, svt_hip_frame_read_coef_host behind test_tile_read_inter.read_frame's."""
import ctypes as C

import numpy as np

import coef_update_model as CM
import entropy_model as E
import frame_model as FM
import modes_inter_model as IM
import svt_testlib as T

B = T.B
NO_REFRESH = dict(refresh_frame_context=0, frame_parallel_decoding_mode=1)     # what the mode takes: nothing a decoder would keep


def host_entropy_coef(pic, fp, lim=None, trailer=b"", counts=False, **over):
    """svt_hip_entropy_picture_coef over a picture dict: entropy_model.host_entropy's answer and probs (1 728 bytes), update (svt_cu_result)"""
    lib = B.load()
    W, H = pic["W"], pic["H"]
    lf = np.ascontiguousarray(pic["lf_mi"])
    mc = np.ascontiguousarray(pic["mc_mi"]) if pic.get("mc_mi") is not None else None
    q, em = E.aligned16(pic["qcoeff"], np.int16), np.ascontiguousarray(pic["eob_map"], np.uint16)
    cnt = np.full(B.TOK_COUNTS, 7, np.uint32) if counts else None
    s = E.fill_struct(B.EntropyPicture(), (lf.ctypes.data, mc.ctypes.data if mc is not None else None, q.ctypes.data, em.ctypes.data), fp, pic.get("lrf", (1, 3)),
                      pic.get("restrict", 0), trailer, cnt.ctypes.data if counts else None)
    for k, v in over.items():
        setattr(s, k, v)
    lim = lim or E.limits(W, H)
    cap = B.FRAME_UNCOMPRESSED_MAX + hdr_capacity() + int(lim.max_tile_bytes) + 4
    packet = np.full(cap + 16, 0xA5, np.uint8)
    size, res, det = C.c_uint32(0x77777777), np.zeros(1, B.ENTROPY_RESULT_DTYPE), B.EntropyHostDetail()
    probs, update = np.full(1728 + 16, 0xA5, np.uint8), np.zeros(1, B.CU_RESULT_DTYPE)
    tb, tm, ti = E.tables()
    rc = lib.svt_hip_entropy_picture_coef(tb.ctypes.data, tm.ctypes.data, ti.ctypes.data, C.byref(s), lf.shape[1], C.byref(lim), packet.ctypes.data, cap, C.byref(size),
                                          res.ctypes.data, C.byref(det), probs.ctypes.data, update.ctypes.data)
    assert (packet[cap:] == 0xA5).all() and (probs[1728:] == 0xA5).all()
    has = rc == 0 and size.value != B.FRAME_SIZE_NONE
    return dict(rc=rc, packet=bytes(packet[:size.value]) if has else None, size=size.value, result={n: int(res[0][n]) for n in res.dtype.names},
                stream_bools=det.stream_bools, header_bytes=det.header_bytes, coded_size=det.coded_size, counts=cnt, probs=probs[:1728].copy(), update=update[0])


def hdr_capacity():
    lib = B.load()
    return int(lib.svt_hip_boolcode_capacity(lib.svt_hip_coef_update_bools_capacity()))


def entry_picture(kind, pic):
    """a picture of the models as the entry takes it"""
    if kind == "key":
        return dict(W=pic["W"], H=pic["H"], lf_mi=pic["lf_mi"], mc_mi=None, qcoeff=pic["qcoeff"], eob_map=pic["eob_map"])
    return pic


def fixture_cases():
    """[(name, kind, model picture, frame parameters, entry picture)]: the four real-stream pictures, every one sends at least one transform size"""
    return [(name, kind, pic, fp, entry_picture(kind, pic)) for name, kind, pic, fp in CM.real_pictures()]


def read_frame_coef(frame, W, H, restrict=0, lrf=(IM.LAST, IM.ALTREF), stride=None):
    """svt_hip_frame_read_coef_host: (rc, info, the outputs, the table the tile was coded with, the caller's tables untouched)"""
    from test_tile_read_inter import BT, IT, KT, Outputs
    buf = np.frombuffer(bytes(frame), np.uint8).copy()
    out, info = Outputs(W, H, stride or W // 8), B.FrameReadInfo()
    vp = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    mine, tabs = BT.copy(), BT.copy()
    tabs["coef_probs"][0][:] = 0
    rc = B.load().svt_hip_frame_read_coef_host(vp(buf), len(buf), (C.c_int8 * 4)(*FM.DEFAULT_REF_DELTAS), (C.c_int8 * 2)(0, 0), stride or W // 8, restrict, (C.c_uint8 * 2)(*lrf),
                                               vp(mine), vp(KT), vp(IT), C.byref(info), *out.pointers(), vp(tabs))
    return rc, info, out.result(), tabs["coef_probs"][0].reshape(-1).copy(), bool(mine.tobytes() == BT.tobytes())
