/*
 * entropy.hip -- the entropy pass over a batch of pictures (gfx950): one entry from what the encode pass leaves on the device to dense
 * VP9 packets, the counterpart of svt_hip_encdec_batch_device behind it.
 *
 * The driver calls the existing stage entries in their fixed order on the context's stream -- tokeniser, inter mode labelling, the two
 * mode-info stages, bool coder, frame assembly -- over buffers of a workspace sized by the caller's budgets, and puts two small kernels
 * of its own round the bool coder (rules: csrc/entropy_core.h):
 *   svt_ent_gate_kernel     ENT_WGS workgroups per picture (grid.y = picture).  Every lane reads the picture's seven words -- the
 *                           tokeniser's total, the mode-info total, the labelling's four status words -- and derives the verdict
 *                           itself: no LDS, no second launch.  For a verdict that is not 0 the workgroups zero the picture's segment
 *                           list in a grid-stride loop of 16-byte stores (a record is {first, count, kind}: every count becomes 0), so
 *                           the bool coder codes the empty stream and reads neither tokens nor bools.  Lane 0 of workgroup 0 keeps the
 *                           verdict for the second phase.
 *   svt_ent_result_kernel   one workgroup, lane i = picture i, behind the bool coder: STREAM_OVER / TILE_OVER from the tile's size, the
 *                           caller's result record, and SVT_BOOL_SIZE_OVERFLOW over the size of every picture that does not ship, which
 *                           is the frame stage's documented way to give a picture no packet.
 * Coefficient-update mode (svt_hip_entropy_work_set_coef_update, opt-in; off, the calls below are what they were): the forward
 * coefficient-probability update (csrc/coef_update.hip) runs between mode info and the gate over the tokeniser's records and counts, the
 * tiles are coded under every picture's own table, the compressed headers -- now device streams too -- by a second bool-coder call (32
 * pictures make 64 streams, a call takes 32), and svt_hip_frame_parts_batch_device joins uncompressed header, compressed header, tile and
 * trailer.  Every picture is coded against the context's table and independent of the others, so a picture that would make a decoder
 * keep the updated probabilities (!error_resilient_mode && refresh_frame_context) is refused; chaining pictures is out of scope.  A
 * withheld picture is safe: the update stage scans at most max_tokens records, its header stream is coded and ignored; the header stream
 * cannot overflow (csrc/entropy_core.h), so the result kernel and its flags are unchanged.
 * Bounds: the zeroing touches the n_sb * 192 vectors of the picture's own list inside the slab; the result kernel writes n_pics records
 * and n_pics size words.  Plain vector stores, no atomics, no LDS.
 */
#include <hip/hip_runtime.h>
#include <new>
#include "svt_ctx.h"
#include "entropy_core.h"

#ifndef ENT_WGS
#define ENT_WGS 8         /* workgroups per picture: with 256 lanes x 16 bytes, 32 KiB of the list a pass (a 2160p list is 6.2 MB) */
#endif
#define ENT_LANES 256

extern "C" int32_t svt_entropy_check_limits(int32_t width, int32_t height, int32_t mi_stride, const svt_entropy_limits *limits, svt_ent_layout *l);
extern "C" int32_t svt_entropy_check_picture(const svt_entropy_picture *p, int32_t width, int32_t height, uint8_t *header, uint32_t *header_len);
extern "C" int32_t svt_entropy_check_picture_coef(const svt_entropy_picture *p);

/* the coefficient-update mode's host descriptors of a call: the update stage, the compressed headers' streams, every tile's table, the
 * three-part packets.  They live with the workspace's second slab, so the pass with the mode off holds nothing of them */
struct ent_coef_desc {
    svt_cu_picture         cu[SVT_FRAME_MAX_PICS];
    svt_bool_stream        hdr_streams[SVT_FRAME_MAX_PICS];
    const uint8_t         *own_probs[SVT_FRAME_MAX_PICS];
    svt_frame_parts_packet parts[SVT_FRAME_MAX_PICS];
};

struct svt_entropy_work {
    svt_hip_ctx       *ctx;
    int32_t            width, height, mi_stride;
    svt_entropy_limits limits;
    svt_ent_layout     l;
    uint8_t           *slab;
    svt_ent_coef_layout cl;   /* the coefficient-update mode: its slab (null until the mode is first enabled) and the switch */
    uint8_t           *slab2;
    ent_coef_desc     *cd;
    bool               coef;
    void             (*hook)(void *user, int32_t stage);
    void              *hook_user;
};

#define ENT_STAGE(k) do { if (w->hook) w->hook(w->hook_user, (k)); } while (0)

namespace {

struct ent_pic_dev {
    const uint32_t     *tok_total, *n_bools, *status; /* status: null for an intra-only picture */
    uint4              *segs;
    uint32_t           *size, *verdict;
    svt_entropy_result *result;
    uint32_t            bools_capacity, pad_;
};
struct ent_batch_dev {
    ent_pic_dev pic[SVT_FRAME_MAX_PICS];
    uint32_t    max_tokens, max_tile_bytes, n_vec; /* n_vec: 16-byte vectors of a segment list */
    int32_t     n_pics;
};

__global__ __launch_bounds__(ENT_LANES) void svt_ent_gate_kernel(const ent_batch_dev *__restrict__ B) {
    const ent_pic_dev &P = B->pic[blockIdx.y];
    const uint32_t     verdict = svt_ent_verdict_a(*P.tok_total, B->max_tokens, *P.n_bools, P.bools_capacity, svt_ent_status_of(P.status));
    if (blockIdx.x == 0 && threadIdx.x == 0) *P.verdict = verdict;
    if (!verdict) return;
    const uint4    zero = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t n_vec = B->n_vec;
    for (uint32_t v = blockIdx.x * ENT_LANES + threadIdx.x; v < n_vec; v += ENT_WGS * ENT_LANES) P.segs[v] = zero;
}

__global__ __launch_bounds__(64) void svt_ent_result_kernel(const ent_batch_dev *__restrict__ B) {
    const int pic = (int)threadIdx.x;
    if (pic >= B->n_pics) return;
    const ent_pic_dev &P = B->pic[pic];
    const uint32_t     size = *P.size, flags = svt_ent_verdict_b(*P.verdict, size, B->max_tile_bytes);
    svt_entropy_result r;
    const uint32_t     out = svt_ent_result_of(flags, *P.tok_total, *P.n_bools, size, svt_ent_status_of(P.status), &r);
    uint32_t *const    d = (uint32_t *)P.result;
    d[0] = r.flags; d[1] = r.tokens; d[2] = r.mode_bools; d[3] = r.tile_bytes;
    d[4] = r.inter_leaves; d[5] = r.newmv_leaves; d[6] = r.unfaithful_leaves; d[7] = 0u;
    if (flags) *P.size = out;
}

void buffers_of(const svt_entropy_work *w, int pic, svt_entropy_buffers *b) {
    uint8_t *const  base = w->slab + (size_t)pic * (size_t)w->l.bytes;
    uint32_t *const words = (uint32_t *)(base + w->l.words);
    b->d_tok_off = (uint32_t *)(base + w->l.tok_off); b->d_sb_off = (uint32_t *)(base + w->l.sb_off); b->d_tokens = (uint32_t *)(base + w->l.tokens);
    b->d_ext = (svt_mi_inter_ext *)(base + w->l.ext); b->d_status = words + SVT_ENT_W_STATUS; b->d_bools = (uint16_t *)(base + w->l.bools);
    b->d_segments = (svt_bool_segment *)(base + w->l.segments); b->d_n_bools = words + SVT_ENT_W_N_BOOLS; b->d_tile = base + w->l.tile;
    b->d_tile_size = words + SVT_ENT_W_SIZE; b->d_verdict = words + SVT_ENT_W_VERDICT;
    b->n_segments = w->l.n_segments; b->n_sb = (uint32_t)w->l.n_sb;
}

void coef_buffers_of(const svt_entropy_work *w, int pic, svt_entropy_coef_buffers *b) {
    uint8_t *const  base = w->slab2 + (size_t)pic * (size_t)w->cl.bytes;
    uint32_t *const words = (uint32_t *)(base + w->cl.words);
    b->d_counts = (uint32_t *)(base + w->cl.counts); b->d_eob_branch = (uint32_t *)(base + w->cl.eob_branch); b->d_probs = base + w->cl.probs;
    b->d_hdr_bools = (uint16_t *)(base + w->cl.hdr_bools); b->d_hdr_bytes = base + w->cl.hdr_bytes; b->d_result = (svt_cu_result *)(base + w->cl.result);
    b->d_n_hdr_bools = words + SVT_ENT_CW_N_HDR_BOOLS; b->d_segment = (svt_bool_segment *)(words + SVT_ENT_CW_SEGMENT); b->d_hdr_size = words + SVT_ENT_CW_HDR_SIZE;
    b->hdr_bools_capacity = SVT_ENT_HDR_BOOLS; b->hdr_capacity = SVT_ENT_HDR_BYTES;
}

} // namespace

extern "C" int32_t svt_hip_entropy_work_create(svt_hip_ctx *ctx, int32_t width, int32_t height, int32_t mi_stride, const svt_entropy_limits *limits,
                                               svt_entropy_work **work) {
    svt_ent_layout l;
    if (!ctx || !work || svt_entropy_check_limits(width, height, mi_stride, limits, &l)) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "entropy: bad workspace argument");
    *work = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    svt_entropy_work *w = new (std::nothrow) svt_entropy_work();
    if (!w) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "entropy: workspace");
    w->ctx = ctx; w->width = width; w->height = height; w->mi_stride = mi_stride; w->limits = *limits; w->l = l;
    svt_ent_coef_layout_of(&w->cl);
    const size_t bytes = (size_t)l.bytes * limits->max_pics;
    if (hipMalloc((void **)&w->slab, bytes) != hipSuccess) {
        (void)hipGetLastError();
        delete w;
        return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "entropy: workspace slab");
    }
    *work = w;
    return SVT_HIP_OK;
}

extern "C" void svt_hip_entropy_work_destroy(svt_hip_ctx *ctx, svt_entropy_work *w) {
    if (!w) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream); /* (a call in flight may still use the slab) */
    }
    (void)hipFree(w->slab);
    if (w->slab2) (void)hipFree(w->slab2);
    delete w->cd;
    delete w;
}

extern "C" int32_t svt_hip_entropy_work_set_coef_update(svt_hip_ctx *ctx, svt_entropy_work *w, int32_t on) {
    if (!ctx || !w || w->ctx != ctx) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "entropy: bad argument");
    if (on && !w->slab2) {
        if (!w->cd && !(w->cd = new (std::nothrow) ent_coef_desc)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "entropy: coefficient-update descriptors");
        HIP_TRY(hipSetDevice(ctx->device));
        if (hipMalloc((void **)&w->slab2, (size_t)w->cl.bytes * w->limits.max_pics) != hipSuccess) {
            (void)hipGetLastError();
            w->slab2 = nullptr;
            return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "entropy: coefficient-update slab");
        }
    }
    w->coef = on != 0;
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_entropy_work_coef_buffers(const svt_entropy_work *w, int32_t pic, svt_entropy_coef_buffers *out) {
    if (!w || !out || !w->slab2 || pic < 0 || (uint32_t)pic >= w->limits.max_pics) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "entropy: bad argument");
    coef_buffers_of(w, pic, out);
    return SVT_HIP_OK;
}

extern "C" void svt_hip_entropy_work_set_stage_hook(svt_entropy_work *w, void (*hook)(void *user, int32_t stage), void *user) {
    if (!w) return;
    w->hook = hook;
    w->hook_user = user;
}

extern "C" int32_t svt_hip_entropy_work_buffers(const svt_entropy_work *w, int32_t pic, svt_entropy_buffers *out) {
    if (!w || !out || pic < 0 || (uint32_t)pic >= w->limits.max_pics) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "entropy: bad argument");
    buffers_of(w, pic, out);
    return SVT_HIP_OK;
}

extern "C" int32_t svt_hip_entropy_batch_device(svt_hip_ctx *ctx, svt_entropy_work *w, int32_t n_pics, const svt_entropy_picture *pics, uint8_t *d_arena,
                                                uint32_t arena_capacity, svt_frame_entry *d_table, svt_entropy_result *d_results) {
    if (!ctx || !w || w->ctx != ctx || !pics || !d_table || !d_results || ((uintptr_t)d_results & 3) || (!d_arena && arena_capacity) || n_pics < 1 ||
        (uint32_t)n_pics > w->limits.max_pics)
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "entropy: bad argument");
    /* everything a stage would refuse, in front of the first launch */
    ENT_STAGE(SVT_ENT_STAGE_HEADERS);
    svt_frame_packet        packets[SVT_FRAME_MAX_PICS];
    svt_tok_picture         tok[SVT_FRAME_MAX_PICS];
    svt_md_inter_picture    label[SVT_FRAME_MAX_PICS];
    svt_modes_picture       key[SVT_FRAME_MAX_PICS];
    svt_modes_inter_picture inter[SVT_FRAME_MAX_PICS];
    svt_bool_stream         streams[SVT_FRAME_MAX_PICS];
    ent_batch_dev           hb;
    int                     n_key = 0, n_inter = 0;
    const bool              coef = w->coef;
    ent_coef_desc *const    cd = coef ? w->cd : nullptr;
    if (coef) memset(cd, 0, sizeof *cd);
    memset(packets, 0, sizeof packets); memset(tok, 0, sizeof tok); memset(label, 0, sizeof label); memset(key, 0, sizeof key);
    memset(inter, 0, sizeof inter); memset(streams, 0, sizeof streams); memset(&hb, 0, sizeof hb);
    for (int i = 0; i < n_pics; i++) {
        const svt_entropy_picture &p = pics[i];
        uint32_t                   header_len = 0;
        if (svt_entropy_check_picture(&p, w->width, w->height, packets[i].header, &header_len)) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "entropy: bad picture");
        svt_entropy_buffers b;
        buffers_of(w, i, &b);
        const bool intra = svt_ent_intra_only(&p.frame) != 0;
        tok[i].d_lf_mi = p.d_lf_mi; tok[i].d_qcoeff = p.d_qcoeff; tok[i].d_eob_map = p.d_eob_map; tok[i].d_tokens = b.d_tokens; tok[i].capacity = w->limits.max_tokens;
        tok[i].d_tok_off = b.d_tok_off; tok[i].d_sb_off = b.d_sb_off; tok[i].d_counts = p.d_counts;
        if (intra) {
            svt_modes_picture &k = key[n_key++];
            k.d_lf_mi = p.d_lf_mi; k.d_eob_map = p.d_eob_map; k.d_tok_off = b.d_tok_off; k.d_bools = b.d_bools; k.d_segments = b.d_segments; k.d_n_bools = b.d_n_bools;
            k.capacity = w->l.kf_bools;
        } else {
            svt_md_inter_picture &d = label[n_inter];
            d.d_lf_mi = p.d_lf_mi; d.d_mc_mi = p.d_mc_mi; d.d_ext_out = b.d_ext; d.d_status = b.d_status;
            memcpy(d.list_ref_frame, p.list_ref_frame, 2);
            memcpy(d.ref_frame_sign_bias, p.frame.ref_frame_sign_bias, 4);
            d.restrict_ref_mvs = p.restrict_ref_mvs; d.allow_hp = p.frame.allow_hp; d.reference_mode = p.frame.reference_mode;
            svt_ent_compound_refs(p.frame.ref_frame_sign_bias, &d.comp_fixed_ref, d.comp_var_ref);
            svt_modes_inter_picture &m = inter[n_inter++];
            m.d_lf_mi = p.d_lf_mi; m.d_eob_map = p.d_eob_map; m.d_tok_off = b.d_tok_off; m.d_bools = b.d_bools; m.d_segments = b.d_segments; m.d_n_bools = b.d_n_bools;
            m.capacity = w->l.inter_bools; m.d_mc_mi = p.d_mc_mi; m.d_ext = b.d_ext;
            m.reference_mode = d.reference_mode; m.allow_hp = d.allow_hp; m.comp_fixed_ref = d.comp_fixed_ref;
            memcpy(m.comp_var_ref, d.comp_var_ref, 2);
            memcpy(m.ref_frame_sign_bias, d.ref_frame_sign_bias, 4);
        }
        svt_bool_stream &s = streams[i];
        s.d_tokens = b.d_tokens; s.d_bools = b.d_bools; s.d_segments = b.d_segments; s.d_n_tokens = b.d_sb_off + w->l.n_sb; s.n_segments = b.n_segments;
        s.max_bools = w->limits.max_bools; s.capacity = w->limits.max_tile_bytes; s.d_bytes = b.d_tile; s.d_size = b.d_tile_size;
        svt_frame_packet &q = packets[i];
        q.d_tile = b.d_tile; q.d_tile_size = b.d_tile_size; q.tile_capacity = w->limits.max_tile_bytes; q.header_len = (uint8_t)header_len;
        q.trailer_len = p.trailer_len;
        memcpy(q.trailer, p.trailer, 4);
        if (coef) {
            svt_entropy_coef_buffers c;
            coef_buffers_of(w, i, &c);
            svt_frame_parts_packet &t = cd->parts[i];
            svt_cu_picture         &u = cd->cu[i];
            uint32_t                ub = 0, size_bit = 0, n_prefix = 0, n_suffix = 0;
            if (svt_entropy_check_picture_coef(&p))
                return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "entropy: the coefficient-update mode does not take a picture with !error_resilient_mode && refresh_frame_context");
            if (svt_hip_frame_header_uncompressed_host(&p.frame, t.header, SVT_FRAME_UNCOMPRESSED_MAX, &ub, &size_bit) ||
                svt_hip_frame_header_parts_host(&p.frame, u.prefix, &n_prefix, u.suffix, &n_suffix))
                return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "entropy: bad picture (frame parameters the header writers refuse)");
            if (!p.d_counts) tok[i].d_counts = c.d_counts; /* the stage needs counts */
            u.d_tokens = b.d_tokens; u.d_n_tokens = b.d_sb_off + w->l.n_sb; u.d_counts = tok[i].d_counts; u.d_eob_branch = c.d_eob_branch; u.d_probs = c.d_probs;
            u.d_hdr_bools = c.d_hdr_bools; u.d_n_hdr_bools = c.d_n_hdr_bools; u.d_segment = c.d_segment; u.d_result = c.d_result;
            u.max_tokens = w->limits.max_tokens; u.n_prefix = (uint16_t)n_prefix; u.n_suffix = (uint16_t)n_suffix;
            svt_bool_stream &h = cd->hdr_streams[i];
            h.d_bools = c.d_hdr_bools; h.d_segments = c.d_segment; h.n_segments = 1; h.max_bools = c.hdr_bools_capacity; h.capacity = c.hdr_capacity;
            h.d_bytes = c.d_hdr_bytes; h.d_size = c.d_hdr_size;
            cd->own_probs[i] = c.d_probs;
            t.d_compressed = c.d_hdr_bytes; t.d_compressed_size = c.d_hdr_size; t.compressed_capacity = c.hdr_capacity;
            t.d_tile = b.d_tile; t.d_tile_size = b.d_tile_size; t.tile_capacity = w->limits.max_tile_bytes;
            t.size_bit = (uint16_t)size_bit; t.header_len = (uint8_t)ub; t.trailer_len = p.trailer_len;
            memcpy(t.trailer, p.trailer, 4);
        }
        ent_pic_dev &P = hb.pic[i];
        P.tok_total = b.d_sb_off + w->l.n_sb; P.n_bools = b.d_n_bools; P.status = intra ? nullptr : b.d_status; P.segs = (uint4 *)b.d_segments; P.size = b.d_tile_size;
        P.verdict = b.d_verdict; P.result = d_results + i; P.bools_capacity = intra ? w->l.kf_bools : w->l.inter_bools;
    }
    hb.max_tokens = w->limits.max_tokens; hb.max_tile_bytes = w->limits.max_tile_bytes; hb.n_vec = w->l.n_segments / 4 * 3; hb.n_pics = n_pics;
    if (!ctx->slot_bytes[SVT_SLOT_BC_TABLES] || (n_key && !ctx->slot_bytes[SVT_SLOT_MI_TABLES]) || (n_inter && !ctx->slot_bytes[SVT_SLOT_MII_TABLES]))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "entropy: the bool coder's or a mode-info stage's tables have not been set");
    HIP_TRY(hipSetDevice(ctx->device));

    int32_t rc;
    ENT_STAGE(SVT_ENT_STAGE_TOKENS);
    if ((rc = svt_hip_tokenize_batch_device(ctx, n_pics, tok, w->width, w->height, w->mi_stride))) return rc;
    ENT_STAGE(SVT_ENT_STAGE_LABELS);
    if (n_inter && (rc = svt_hip_md_inter_modes_batch_device(ctx, n_inter, label, w->width, w->height, w->mi_stride))) return rc;
    ENT_STAGE(SVT_ENT_STAGE_MODES);
    if (n_key && (rc = svt_hip_modes_kf_batch_device(ctx, n_key, key, w->width, w->height, w->mi_stride))) return rc;
    if (n_inter && (rc = svt_hip_modes_inter_batch_device(ctx, n_inter, inter, w->width, w->height, w->mi_stride))) return rc;
    if (coef) {
        ENT_STAGE(SVT_ENT_STAGE_COEF_UPDATE);
        if ((rc = svt_hip_coef_update_batch_device(ctx, n_pics, cd->cu))) return rc;
    }
    ENT_STAGE(SVT_ENT_STAGE_GATE);
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof hb, &h, &d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "entropy: descriptor buffers");
    memcpy(h, &hb, sizeof hb);
    HIP_TRY(svt_ctx_stage_send(ctx, sizeof hb));
    const ent_batch_dev *dB = (const ent_batch_dev *)d; /* both phases read it: the slot is not taken again before 63 further uploads, each behind these kernels on the stream */
    hipLaunchKernelGGL(svt_ent_gate_kernel, dim3(ENT_WGS, (unsigned)n_pics), dim3(ENT_LANES), 0, ctx->stream, dB);
    HIP_TRY(hipGetLastError());
    ENT_STAGE(SVT_ENT_STAGE_BOOLCODE);
    if (!coef) {
        if ((rc = svt_hip_boolcode_batch_device(ctx, n_pics, streams))) return rc;
    } else { /* the tiles under every picture's own table; then the compressed headers: 32 pictures make 64 streams, one call takes 32 */
        if ((rc = svt_hip_boolcode_batch_tables_device(ctx, n_pics, streams, cd->own_probs))) return rc;
        if ((rc = svt_hip_boolcode_batch_device(ctx, n_pics, cd->hdr_streams))) return rc;
    }
    ENT_STAGE(SVT_ENT_STAGE_RESULT);
    hipLaunchKernelGGL(svt_ent_result_kernel, dim3(1), dim3(64), 0, ctx->stream, dB);
    HIP_TRY(hipGetLastError());
    ENT_STAGE(SVT_ENT_STAGE_FRAME);
    if ((rc = coef ? svt_hip_frame_parts_batch_device(ctx, n_pics, cd->parts, d_arena, arena_capacity, d_table)
                   : svt_hip_frame_batch_device(ctx, n_pics, packets, d_arena, arena_capacity, d_table)))
        return rc;
    ENT_STAGE(SVT_ENT_STAGE_END);
    return SVT_HIP_OK;
}
