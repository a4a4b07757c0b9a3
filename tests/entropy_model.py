"""Shared by the entropy-pass tests (test_entropy_host.py, test_gpu_entropy.py): pictures as the entry takes them, frame parameters for the
fixtures' pictures, the host form svt_hip_entropy_picture behind a numpy interface, the limits."""
import ctypes as C

import numpy as np

import boolcode_model as BM
import frame_model as FM
import md_inter_model as D
import modes_inter_model as IM
import modes_model as MM
import svt_testlib as T

B = T.B


def readable(sign_bias):
    """the decoder's condition for reading the reference-mode bits"""
    return int(sign_bias[2] != sign_bias[1] or sign_bias[3] != sign_bias[1])


def key_params(W, H, **kw):
    return FM.params(width=W, height=H, **kw)


def inter_params(pic, **kw):
    """frame parameters an inter picture of the md_inter / modes_inter models is coded under"""
    fr = pic["frame"]
    v = dict(width=pic["W"], height=pic["H"], reference_mode=fr["reference_mode"], allow_hp=fr["allow_hp"], ref_frame_sign_bias=tuple(fr["sign_bias"]),
             allow_comp_inter_inter=readable(fr["sign_bias"]))
    v.update(kw)
    return FM.inter(**v)


def key_picture(name):
    """a key picture of tests/golden/modes_reference.npz as the entry takes it"""
    p = MM.fixture_picture(name)
    return dict(W=p["W"], H=p["H"], lf_mi=p["lf_mi"], mc_mi=None, qcoeff=p["qcoeff"], eob_map=p["eob_map"], tile=p["tile"])


def zero_coefficients(pic):
    """a picture of grids alone (every leaf skipped) with the coefficient arrays the entry wants"""
    W, H = pic["W"], pic["H"]
    return dict(pic, qcoeff=np.zeros(T.n_sb(W, H) * B.SB_COEFFS, np.int16), eob_map=np.zeros(W * H * 3 // 32, np.uint16))


def aligned16(a, dtype):
    """a contiguous copy whose first byte lies on a 16-byte boundary"""
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    raw = np.empty(a.nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    out = raw[off:off + a.nbytes].view(dtype)
    out[:] = a
    return out


def limits(W, H, n_pics=1, **over):
    lim = B.EntropyLimits()
    B.load().svt_hip_entropy_limits_worst(W, H, n_pics, C.byref(lim))
    for k, v in over.items():
        setattr(lim, k, v)
    return lim


def fill_struct(s, ptrs, fp, lrf=(1, 3), restrict=0, trailer=b"", counts=None):
    """ptrs: (lf_mi, mc_mi or None, qcoeff, eob_map) addresses; fp: a frame_model parameter set or a B.FrameParams"""
    s.d_lf_mi, s.d_mc_mi, s.d_qcoeff, s.d_eob_map = ptrs
    s.d_counts = counts
    s.frame = fp if isinstance(fp, B.FrameParams) else FM.struct(fp)
    s.list_ref_frame[0], s.list_ref_frame[1] = lrf
    s.restrict_ref_mvs, s.trailer_len = restrict, len(trailer)
    for i, v in enumerate(trailer[:4]):
        s.trailer[i] = v
    return s


_tables = None


def tables():
    global _tables
    if _tables is None:
        _tables = (BM.tables()[1], MM.tables()[1], IM.tables()[1])
    return _tables


def host_entropy(pic, fp, lim=None, trailer=b"", counts=False, **over):
    """svt_hip_entropy_picture over a picture dict (W, H, lf_mi [rows, mi_stride], mc_mi or None, qcoeff, eob_map, lrf, restrict) ->
    dict(rc, packet: bytes or None, size, result: dict, stream_bools, header_bytes, coded_size, counts)"""
    lib = B.load()
    W, H = pic["W"], pic["H"]
    lf = np.ascontiguousarray(pic["lf_mi"])
    mc = np.ascontiguousarray(pic["mc_mi"]) if pic.get("mc_mi") is not None else None
    q, em = aligned16(pic["qcoeff"], np.int16), np.ascontiguousarray(pic["eob_map"], np.uint16)
    cnt = np.full(B.TOK_COUNTS, 7, np.uint32) if counts else None
    s = fill_struct(B.EntropyPicture(), (lf.ctypes.data, mc.ctypes.data if mc is not None else None, q.ctypes.data, em.ctypes.data), fp, pic.get("lrf", (1, 3)),
                    pic.get("restrict", 0), trailer, cnt.ctypes.data if counts else None)
    for k, v in over.items():
        setattr(s, k, v)
    lim = lim or limits(W, H)
    cap = B.FRAME_HEADER_MAX + int(lim.max_tile_bytes) + 4
    packet = np.full(cap + 16, 0xA5, np.uint8)
    size, res, det = C.c_uint32(0x77777777), np.zeros(1, B.ENTROPY_RESULT_DTYPE), B.EntropyHostDetail()
    tb, tm, ti = tables()
    rc = lib.svt_hip_entropy_picture(tb.ctypes.data, tm.ctypes.data, ti.ctypes.data, C.byref(s), lf.shape[1], C.byref(lim), packet.ctypes.data, cap, C.byref(size),
                                     res.ctypes.data, C.byref(det))
    assert (packet[cap:] == 0xA5).all()
    has = rc == 0 and size.value != B.FRAME_SIZE_NONE
    return dict(rc=rc, packet=bytes(packet[:size.value]) if has else None, size=size.value, result={n: int(res[0][n]) for n in res.dtype.names},
                stream_bools=det.stream_bools, header_bytes=det.header_bytes, coded_size=det.coded_size, counts=cnt)


def gate(tok_total, max_tokens, n_bools, bools_capacity, status, size, max_tile_bytes):
    """svt_hip_entropy_gate_host -> (phase A's verdict, the flags, what the size word becomes, the result record)"""
    st = np.asarray(status, np.uint32) if status is not None else None
    a, res = C.c_uint32(0x77), np.zeros(1, B.ENTROPY_RESULT_DTYPE)
    out = B.load().svt_hip_entropy_gate_host(tok_total, max_tokens, n_bools, bools_capacity, st.ctypes.data if st is not None else None, size, max_tile_bytes,
                                             C.byref(a), res.ctypes.data)
    return a.value, int(res[0]["flags"]), int(out), {n: int(res[0][n]) for n in res.dtype.names}


def golden_inter(name):
    """(picture, frame parameters, the expected packet) of a picture of tests/golden/md_inter_reference.npz: host header || the reference's tile"""
    p = D.golden_picture(name)
    fp = inter_params(p)
    return p, fp, FM.host_header_bytes(fp) + p["tile"]


def empty_stream_bytes():
    """what the bool coder writes for a stream without a record"""
    return BM.host_code(tokens=np.zeros(0, np.uint32))[0]
