"""Python model of the frame stage, written independently of the C text (host/frame_host.c, csrc/frame_core.h):
  - headers(): the VP9 uncompressed header through a plain bit writer and the compressed header as bools through
    boolcode_model.serial_write, from a dict of frame parameters;
  - the named header cases and the whole-frame cases the fixture (tests/golden/frame_reference.npz), the CPU tests and the GPU tests
    share, the seeded sweep of valid parameter sets;
  - the seeded packet batches of the assembly tests and their numpy concatenation."""
import ctypes as C
import os

import numpy as np

import boolcode_model as BM
import svt_testlib as T

B = T.B
GOLD = os.path.join(T.GOLDEN_DIR, "frame_reference.npz")
KEY, INTER = 0, 1
SINGLE, COMPOUND, SELECT = 0, 1, 2
# every field of svt_frame_params, in the order the fixture and the reference's driver hold them (arrays flattened)
FIELDS = ("frame_type", "show_frame", "error_resilient_mode", "intra_only", "reset_frame_context", "refresh_frame_context", "frame_parallel_decoding_mode",
          "frame_context_idx", "refresh_frame_mask", "ref_dpb_index", "ref_frame_sign_bias", "allow_hp", "reference_mode", "allow_comp_inter_inter",
          "color_space", "color_range", "width", "height", "render_width", "render_height", "filter_level", "sharpness_level", "mode_ref_delta_enabled",
          "mode_ref_delta_update", "ref_deltas", "mode_deltas", "last_ref_deltas", "last_mode_deltas", "base_qindex", "y_dc_delta_q", "uv_dc_delta_q",
          "uv_ac_delta_q")
ARRAYS = dict(ref_dpb_index=3, ref_frame_sign_bias=4, ref_deltas=4, mode_deltas=2, last_ref_deltas=4, last_mode_deltas=2)
N_VALUES = sum(ARRAYS.get(f, 1) for f in FIELDS)
# the reference's stream defaults (vp9_default_lf_deltas sets ref_deltas 1, 0, -1, -1 and mode_deltas 0, 0)
DEFAULT_REF_DELTAS = (1, 0, -1, -1)


def params(**kw):
    """a parameter set: a shown key frame of 64x64 at qindex 120 unless told otherwise; render size follows the coded size"""
    p = dict(frame_type=KEY, show_frame=1, error_resilient_mode=0, intra_only=0, reset_frame_context=0, refresh_frame_context=1, frame_parallel_decoding_mode=0,
             frame_context_idx=0, refresh_frame_mask=0xFF, ref_dpb_index=(0, 1, 2), ref_frame_sign_bias=(0, 0, 0, 0), allow_hp=0, reference_mode=SINGLE,
             allow_comp_inter_inter=0, color_space=2, color_range=0, width=64, height=64, render_width=None, render_height=None, filter_level=20,
             sharpness_level=0, mode_ref_delta_enabled=0, mode_ref_delta_update=0, ref_deltas=DEFAULT_REF_DELTAS, mode_deltas=(0, 0),
             last_ref_deltas=DEFAULT_REF_DELTAS, last_mode_deltas=(0, 0), base_qindex=120, y_dc_delta_q=0, uv_dc_delta_q=0, uv_ac_delta_q=0)
    assert set(kw) <= set(p), set(kw) - set(p)
    p.update(kw)
    if p["render_width"] is None:
        p["render_width"] = p["width"]
    if p["render_height"] is None:
        p["render_height"] = p["height"]
    return p


def inter(**kw):
    return params(**{**dict(frame_type=INTER, refresh_frame_mask=0x01), **kw})


# (name, parameters): the issue's groups 1 .. 9
CASES = (
    ("key", params()),
    ("intra_only_hidden", params(frame_type=INTER, show_frame=0, intra_only=1, reset_frame_context=2, refresh_frame_mask=0x12)),
    ("inter_single", inter()),
    ("inter_single_comp_allowed", inter(allow_comp_inter_inter=1)),
    ("inter_hidden", inter(show_frame=0)),
    ("inter_compound", inter(reference_mode=COMPOUND, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1))),
    ("inter_select_altref_bias", inter(reference_mode=SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1))),
    ("inter_hp", inter(allow_hp=1)),
    ("inter_select_hp", inter(allow_hp=1, reference_mode=SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 1, 1))),
    ("key_error_resilient", params(error_resilient_mode=1, reset_frame_context=0)),
    ("inter_error_resilient", inter(error_resilient_mode=1, frame_context_idx=3, frame_parallel_decoding_mode=1)),
    ("inter_context_flags", inter(reset_frame_context=3, refresh_frame_context=0, frame_parallel_decoding_mode=1, frame_context_idx=2)),
    ("q0", params(base_qindex=0)),
    ("q255", params(base_qindex=255)),
    ("chroma_dq_minus15", params(uv_dc_delta_q=-15, uv_ac_delta_q=-15)),
    ("dq_plus15", params(y_dc_delta_q=15, uv_dc_delta_q=15, uv_ac_delta_q=7)),
    ("lf_0", params(filter_level=0)),
    ("lf_63_sharp7", params(filter_level=63, sharpness_level=7)),
    ("lf_deltas_no_update", inter(mode_ref_delta_enabled=1)),
    ("lf_deltas_update_mixed", inter(mode_ref_delta_enabled=1, mode_ref_delta_update=1, ref_deltas=(1, -5, -1, 63), mode_deltas=(0, -63), last_mode_deltas=(0, 0))),
    ("lf_deltas_update_none_changed", params(mode_ref_delta_enabled=1, mode_ref_delta_update=1)),
    ("refresh_00_dpb_0", inter(refresh_frame_mask=0x00, ref_dpb_index=(0, 0, 0))),
    ("refresh_ff_dpb_7", inter(refresh_frame_mask=0xFF, ref_dpb_index=(7, 7, 7))),
    ("dpb_mixed", inter(refresh_frame_mask=0xA5, ref_dpb_index=(3, 0, 7), ref_frame_sign_bias=(0, 1, 0, 1))),
    ("render_differs_key", params(width=72, height=40, render_width=70, render_height=38)),
    ("render_differs_inter", inter(width=72, height=40, render_width=65536, render_height=1)),
    ("width_64", params(width=64, height=8)),
    ("width_448", params(width=448, height=64)),
    ("width_449", params(width=449, height=64)),
    ("width_504", params(width=504, height=64)),
    ("width_512", inter(width=512, height=64)),
    ("width_4096", params(width=4096, height=2160)),
    ("width_4096_inter_tall", inter(width=4096, height=65536)),
    ("width_1_height_1", params(width=1, height=1)),
    ("color_space_0", params(color_space=0)),
    ("color_space_2_full_range", params(color_space=2, color_range=1)),
    ("color_space_6", params(color_space=6, color_range=1)),
)
SHOW_EXISTING_SLOTS = (0, 3, 7)
# group 11: (name, fixture, picture, parameters): the fixture's recorded tile bytes as the entropy coder's stream
WHOLE = (
    ("whole_key_a", "modes", "edge_72x40_a", params(width=72, height=40)),
    ("whole_key_b", "modes", "edge_72x40_b", params(width=72, height=40, base_qindex=60, uv_dc_delta_q=-15, uv_ac_delta_q=-15)),
    ("whole_inter_single", "modes_inter", "edge_72x40_a", inter(width=72, height=40)),
    ("whole_inter_select", "modes_inter", "edge_72x40_b", inter(width=72, height=40, reference_mode=SELECT, allow_comp_inter_inter=1, ref_frame_sign_bias=(0, 0, 0, 1),
                                                               refresh_frame_mask=0x04, ref_dpb_index=(0, 1, 2))),
)


def whole_tile(kind, picture):
    if kind == "modes":
        import modes_model as MM
        return MM.fixture_picture(picture)["tile"]
    import modes_inter_model as IM
    p = IM.fixture_picture(picture)
    return p["tile"]


def flat(p):
    """the parameter set as N_VALUES integers in FIELDS' order"""
    out = []
    for f in FIELDS:
        out += list(p[f]) if f in ARRAYS else [p[f]]
    assert len(out) == N_VALUES
    return [int(v) for v in out]


def unflat(values):
    p, it = {}, iter(int(v) for v in values)
    for f in FIELDS:
        p[f] = tuple(next(it) for _ in range(ARRAYS[f])) if f in ARRAYS else next(it)
    return p


def struct(p):
    s = B.FrameParams()
    for f in FIELDS:
        if f in ARRAYS:
            for i, v in enumerate(p[f]):
                getattr(s, f)[i] = v
        else:
            setattr(s, f, p[f])
    return s


# ---------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.bits = []

    def put(self, value, n=1):
        assert 0 <= value < 1 << n, (value, n)
        self.bits += [(value >> (n - 1 - k)) & 1 for k in range(n)]

    def data(self):
        padded = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(int("".join(map(str, padded[i:i + 8])), 2) for i in range(0, len(padded), 8))


def tile_column_bit(width):
    """is increment_tile_cols_log2 coded?  (VP9 specification, tile_info: minLog2 = 0 up to 64 SB columns, maxLog2 > 0 from 8 SB columns)"""
    sb_cols = (((width + 7) // 8) + 7) // 8
    assert sb_cols <= 64
    return sb_cols >= 8


def uncompressed_bits(p, first_part_size):
    """the bit writer behind the uncompressed header, first_part_size its last 16 bits"""
    w = Bits()
    w.put(2, 2)                  # frame_marker
    w.put(0, 1); w.put(0, 1)     # profile_low_bit, profile_high_bit                  # noqa: E702
    w.put(0)                     # show_existing_frame
    w.put(p["frame_type"]); w.put(p["show_frame"]); w.put(p["error_resilient_mode"])   # noqa: E702

    def sync():
        w.put(0x49, 8); w.put(0x83, 8); w.put(0x42, 8)      # noqa: E702

    def size():
        w.put(p["width"] - 1, 16); w.put(p["height"] - 1, 16)      # noqa: E702

    def render():
        differs = (p["render_width"], p["render_height"]) != (p["width"], p["height"])
        w.put(int(differs))
        if differs:
            w.put(p["render_width"] - 1, 16); w.put(p["render_height"] - 1, 16)      # noqa: E702
    if p["frame_type"] == KEY:
        sync()
        w.put(p["color_space"], 3); w.put(p["color_range"])      # noqa: E702
        size(); render()                                         # noqa: E702
    else:
        if not p["show_frame"]:
            w.put(p["intra_only"])
        if not p["error_resilient_mode"]:
            w.put(p["reset_frame_context"], 2)
        if p["intra_only"]:
            sync()
            w.put(p["refresh_frame_mask"], 8)
            size(); render()                                     # noqa: E702
        else:
            w.put(p["refresh_frame_mask"], 8)
            for r in range(3):
                w.put(p["ref_dpb_index"][r], 3); w.put(p["ref_frame_sign_bias"][1 + r])      # noqa: E702
            for r in range(3):
                w.put(0)            # found_ref
            size(); render()        # noqa: E702
            w.put(p["allow_hp"])
            w.put(0); w.put(1, 2)   # is_filter_switchable, raw_interpolation_filter      # noqa: E702
    if not p["error_resilient_mode"]:
        w.put(p["refresh_frame_context"]); w.put(p["frame_parallel_decoding_mode"])      # noqa: E702
    w.put(p["frame_context_idx"], 2)
    w.put(p["filter_level"], 6); w.put(p["sharpness_level"], 3)      # noqa: E702
    w.put(p["mode_ref_delta_enabled"])
    if p["mode_ref_delta_enabled"]:
        w.put(p["mode_ref_delta_update"])
        if p["mode_ref_delta_update"]:
            for new, last in list(zip(p["ref_deltas"], p["last_ref_deltas"])) + list(zip(p["mode_deltas"], p["last_mode_deltas"])):
                w.put(int(new != last))
                if new != last:
                    w.put(abs(new), 6); w.put(int(new < 0))      # noqa: E702
    w.put(p["base_qindex"], 8)
    for dq in (p["y_dc_delta_q"], p["uv_dc_delta_q"], p["uv_ac_delta_q"]):
        w.put(int(dq != 0))
        if dq:
            w.put(abs(dq), 4); w.put(int(dq < 0))      # noqa: E702
    w.put(0)        # segmentation_enabled
    if tile_column_bit(p["width"]):
        w.put(0)
    w.put(0)        # tile_rows_log2
    w.put(first_part_size, 16)
    return w


def uncompressed(p, first_part_size):
    return uncompressed_bits(p, first_part_size).data()


def compressed(p):
    """no forward update anywhere: tx_mode, a 0 per coefficient table, a (252, 0) per probability"""
    lit, no = (lambda b: BM.rec(b, 128)), BM.rec(0, 252)
    out = [lit(1), lit(1), lit(0)] + [lit(0)] * 4 + [no] * 3
    if p["frame_type"] != KEY and not p["intra_only"]:
        out += [no] * (7 * 3 + 4)
        if p["allow_comp_inter_inter"]:
            out.append(lit(int(p["reference_mode"] != SINGLE)))
            if p["reference_mode"] != SINGLE:
                out.append(lit(int(p["reference_mode"] == SELECT)))
                if p["reference_mode"] == SELECT:
                    out += [no] * 5
        if p["reference_mode"] != COMPOUND:
            out += [no] * 10
        if p["reference_mode"] != SINGLE:
            out += [no] * 5
        out += [no] * (4 * 9 + 16 * 3)
        out += [no] * (3 + 2 * 22 + 2 * 9 + (4 if p["allow_hp"] else 0))
    return BM.serial_write(out)


def headers(p):
    """(uncompressed header with first_part_size, compressed header)"""
    c = compressed(p)
    return uncompressed(p, len(c)), c


def show_existing(slot):
    w = Bits()
    w.put(2, 2); w.put(0, 2); w.put(1); w.put(slot, 3)      # noqa: E702
    return w.data()


def random_params(rng):
    """a valid parameter set, every field drawn over its whole range"""
    r = lambda lo, hi: int(rng.integers(lo, hi + 1))      # noqa: E731
    frame_type, show = r(0, 1), r(0, 1)
    w, h = r(1, 4096), r(1, 65536)
    scaled = r(0, 1)
    return params(frame_type=frame_type, show_frame=show, error_resilient_mode=r(0, 1), intra_only=r(0, 1) if frame_type == INTER and not show else 0,
                  reset_frame_context=r(0, 3), refresh_frame_context=r(0, 1), frame_parallel_decoding_mode=r(0, 1), frame_context_idx=r(0, 3),
                  refresh_frame_mask=r(0, 255), ref_dpb_index=tuple(r(0, 7) for _ in range(3)), ref_frame_sign_bias=tuple(r(0, 1) for _ in range(4)),
                  allow_hp=r(0, 1), reference_mode=r(0, 2), allow_comp_inter_inter=r(0, 1), color_space=r(0, 6), color_range=r(0, 1), width=w, height=h,
                  render_width=r(1, 65536) if scaled else w, render_height=r(1, 65536) if scaled else h, filter_level=r(0, 63), sharpness_level=r(0, 7),
                  mode_ref_delta_enabled=r(0, 1), mode_ref_delta_update=r(0, 1), ref_deltas=tuple(r(-63, 63) for _ in range(4)),
                  mode_deltas=tuple(r(-63, 63) for _ in range(2)), last_ref_deltas=tuple(r(-63, 63) for _ in range(4)),
                  last_mode_deltas=tuple(r(-63, 63) for _ in range(2)), base_qindex=r(0, 255), y_dc_delta_q=r(-15, 15), uv_dc_delta_q=r(-15, 15),
                  uv_ac_delta_q=r(-15, 15))


def worst_params():
    """the longest header the syntax allows: a hidden intra-only picture with a render size, six changed deltas, three delta qs, a tile-column
    bit; and the inter picture with the most compressed-header bools"""
    lf = dict(mode_ref_delta_enabled=1, mode_ref_delta_update=1, ref_deltas=(2, 3, 4, 5), mode_deltas=(6, 7), y_dc_delta_q=1, uv_dc_delta_q=-1, uv_ac_delta_q=2,
              width=4096, height=2160, render_width=1, render_height=1)
    return (params(frame_type=INTER, show_frame=0, intra_only=1, **lf),
            inter(show_frame=0, allow_hp=1, reference_mode=SELECT, allow_comp_inter_inter=1, **lf))


# ---------------------------------------------------------------------------------------------------
# the fixture and the product's host entry point
# ---------------------------------------------------------------------------------------------------
_gold = None


def fixture():
    global _gold
    if _gold is None:
        g = np.load(GOLD)
        _gold = {k: g[k] for k in g.files}
    return _gold


def fixture_case(name):
    """(parameters as the fixture holds them, the reference's frame bytes, its uncompressed header's length, its first_part_size)"""
    g = fixture()
    ub, cb = (int(v) for v in g[f"lengths|{name}"])
    return unflat(g[f"params|{name}"]), bytes(g[f"frame|{name}"]), ub, cb


def host_headers(p, capacity=B.FRAME_HEADER_MAX, fill=0xA5):
    """svt_hip_frame_header_host: (rc, the whole output buffer, uncompressed bytes, compressed bytes)"""
    buf = np.full(capacity + 16, fill, np.uint8)
    ub, cb = C.c_uint32(0x77777777), C.c_uint32(0x77777777)
    s = p if isinstance(p, B.FrameParams) else struct(p)
    rc = B.load().svt_hip_frame_header_host(C.byref(s), buf.ctypes.data_as(C.c_void_p), capacity, C.byref(ub), C.byref(cb))
    return rc, buf, ub.value, cb.value


def host_header_bytes(p):
    rc, buf, ub, cb = host_headers(p)
    assert rc == 0, rc
    return bytes(buf[:ub + cb])


# ---------------------------------------------------------------------------------------------------
# packet batches of the assembly tests
# ---------------------------------------------------------------------------------------------------
TILE_SIZES = (0, 1, 3, 15, 16, 17, 31, 33, 255, 4099)
SLOT = 4099 + 16 + 13           # bytes of the source tensor a picture owns: its tile at offset 0 .. 15 and a gap to the next


def make_batch(seed, n_pics=32, first_pair=None):
    """dict(source: the bytes all tiles are carved from, pics: [dict(src_off, size, capacity, header, trailer)]); picture i's tile starts
    src_off = i * SLOT + (0 .. 15) bytes into the source.  first_pair = k: picture i is made to meet the pair number k + i of the 256
    (source offset mod 16, arena offset of the tile's first byte mod 16) = divmod(k + i, 16) -- its tile is not empty and its header's
    length is drawn among the lengths that put the tile there; otherwise everything is drawn freely, empty tiles included"""
    rng = np.random.default_rng(7000 + seed)
    source = rng.integers(0, 256, n_pics * SLOT + 64, dtype=np.uint8)
    pics, off = [], 0
    for i in range(n_pics):
        if first_pair is None:
            size, mis, hl = int(rng.choice(TILE_SIZES)), int(rng.integers(0, 16)), int(rng.integers(1, B.FRAME_HEADER_MAX + 1))
        else:
            mis, at = divmod(first_pair + i, 16)
            size = int(rng.choice(TILE_SIZES[1:]))
            hl = int(rng.choice([h for h in range(1, B.FRAME_HEADER_MAX + 1) if (off + h) % 16 == at]))
        pics.append(dict(src_off=i * SLOT + mis, size=size, capacity=size + int(rng.integers(0, 8)), header=rng.integers(0, 256, hl, dtype=np.uint8).tobytes(),
                         trailer=rng.integers(0, 256, int(rng.integers(0, 5)), dtype=np.uint8).tobytes()))
        off += hl + size + len(pics[-1]["trailer"])
    return dict(source=source, pics=pics)


def standard_batches():
    """the batches the CPU and the GPU tests share.  A batch has at most 32 pictures and a picture meets one pair, so the 256 pairs need
    eight batches: batch b is made for the pairs 32 b .. 32 b + 31 (for a source and an arena that both start on a 16-byte boundary; the
    tests compute the coverage from the addresses they really have); a ninth is drawn freely and has empty tiles"""
    return [make_batch(b, first_pair=32 * b) for b in range(8)] + [make_batch(8)]


def expected(batch):
    """(the dense arena, the table as (n + 1, 2) uint32) by concatenation; a picture whose size is FRAME_SIZE_NONE or above its capacity has no packet"""
    out, table, none = b"", [], 0
    for p in batch["pics"]:
        if p["size"] == B.BOOL_SIZE_OVERFLOW or p["size"] > p["capacity"]:
            table.append((len(out), B.FRAME_SIZE_NONE))
            none += 1
            continue
        pkt = p["header"] + batch["source"][p["src_off"]:p["src_off"] + p["size"]].tobytes() + p["trailer"]
        table.append((len(out), len(pkt)))
        out += pkt
    table.append((len(out), none))
    return out, np.array(table, np.uint32)


def pairs(batch, base_address, arena_address):
    """{(source address mod 16, destination address of the tile's first byte mod 16)} over the batch's non-empty tiles"""
    _, table = expected(batch)
    out = set()
    for p, (off, size) in zip(batch["pics"], table):
        if size != B.FRAME_SIZE_NONE and p["size"]:
            out.add(((base_address + p["src_off"]) % 16, (arena_address + int(off) + len(p["header"])) % 16))
    return out


def packets(batch, tile_address, size_address):
    """the C array of svt_frame_packet: picture i's tile at tile_address + src_off, its size word at size_address + 4 * i"""
    arr = (B.FramePacket * len(batch["pics"]))()
    for i, (q, p) in enumerate(zip(arr, batch["pics"])):
        q.d_tile, q.d_tile_size, q.tile_capacity = tile_address + p["src_off"], size_address + 4 * i, p["capacity"]
        q.header_len, q.trailer_len = len(p["header"]), len(p["trailer"])
        C.memmove(q.header, p["header"], len(p["header"]))
        C.memmove(q.trailer, p["trailer"], len(p["trailer"]))
    return arr


def sizes_array(batch):
    return np.array([p["size"] for p in batch["pics"]], np.uint32)
