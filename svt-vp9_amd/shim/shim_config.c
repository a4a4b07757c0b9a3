/*
 * shim_config.c -- the configuration rules of the reference behind eb_vp9_svt_init_handle / eb_vp9_svt_enc_set_parameter: the defaults
 * (Codec/EbEncHandle.c:1762-1818), copy_api_from_app (:2052-2192) and verify_settings (:2203-2557).  No device behind them.
 */
#include <stdlib.h>

#include "shim_internal.h"

/* VP9 level limits (max luma picture size, max luma sample rate), indexed like the reference's tables (:109-134) */
static const uint64_t k_max_pic_size[13]    = {36864, 122880, 245760, 552960, 983040, 2228224, 2228224, 8912896, 8912896, 8912896, 35651584, 35651584, 35651584};
static const uint64_t k_max_sample_rate[13] = {552960, 3686400, 7372800, 16588800, 33177600, 66846720, 133693440, 267386880, 534773760,
                                               1069547520ull, 1069547520ull, 2139095040ull, 4278190080ull};

void shim_load_defaults(EbSvtVp9EncConfiguration *c) { /* eb_vp9_svt_enc_init_parameter, :1762-1818 */
    c->frame_rate = 30 << 16; c->frame_rate_numerator = 0; c->frame_rate_denominator = 0;
    c->encoder_bit_depth = 8; c->source_width = 0; c->source_height = 0;
    c->qp = 50; c->use_qp_file = 0; c->rate_control_mode = 0; c->target_bit_rate = 7000000;
    c->max_qp_allowed = 63; c->min_qp_allowed = 0; c->base_layer_switch_mode = 0;
    c->enc_mode = 3; c->intra_period = 31; c->pred_structure = 2;
    c->loop_filter = 1; c->use_default_me_hme = 1; c->enable_hme_flag = 1;
    c->search_area_width = 16; c->search_area_height = 7;
    c->profile = 0; c->level = 0;
    c->injector_frame_rate = 60 << 16; c->speed_control_flag = 0;
    c->asm_type = 1;
    c->logical_processors = 0; c->target_socket = -1; c->channel_id = 0; c->active_channel_count = 1;
    c->recon_file = 0;
}

static int level_index(uint32_t level) {
    static const uint32_t ids[13] = {10, 20, 21, 30, 31, 40, 41, 50, 51, 52, 60, 61, 62};
    if (level == 0) return 13; /* decided by the encoder */
    for (int i = 0; i < 13; i++) if (ids[i] == level) return i;
    return 14;
}

/* verify_settings (:2203-2557) on the values copy_api_from_app (:2052-2164) hands it */
static EbErrorType verify(const EbSvtVp9EncConfiguration *in) {
    EbSvtVp9EncConfiguration c = *in;
    if (c.rate_control_mode == 0) { c.max_qp_allowed = 63; c.min_qp_allowed = 0; } /* :2118-2126 */
    int bad = 0;
    const uint32_t W = c.source_width, H = c.source_height;
    const int li = level_index(c.level);
    if (li > 13) bad = 1;
    if (W < 64 || H < 64) bad = 1;
    if (c.pred_structure != 2) bad = 1;
    if ((W % 2) || (H % 2)) bad = 1;
    if (W > 8192 || (W % 8) || H > 4320 || (H % 8)) bad = 1;
    const int res = svt_hip_input_resolution((int32_t)W, (int32_t)H);
    if (res <= 1) { if (c.enc_mode > 9) bad = 1; }
    else if (res == 2) { if (c.enc_mode > 10) bad = 1; }
    else if ((c.enc_mode > 12 && c.tune == 0) || (c.enc_mode > 10 && c.tune >= 1)) bad = 1;
    if (c.qp > 63) bad = 1;
    if (c.intra_period < -2 || c.intra_period > 255) bad = 1;
    if (c.base_layer_switch_mode > 1 || c.loop_filter > 1 || c.use_default_me_hme > 1 || c.enable_hme_flag > 1) bad = 1;
    if (c.search_area_width > 256 || c.search_area_width == 0 || c.search_area_height > 256 || c.search_area_height == 0) bad = 1;
    if (li < 13) {
        if ((uint64_t)W * H > k_max_pic_size[li]) bad = 1;
        if ((uint64_t)c.frame_rate * W * H > (k_max_sample_rate[li] << 16)) bad = 1;
    }
    if (c.frame_rate > (240u << 16) || c.frame_rate == 0) bad = 1;
    if (c.rate_control_mode > 2) bad = 1;
    /* (the "no rate control in the OQ / VMAF tunes" rule is compiled out in the reference: #if !VP9_RC, :2495-2502) */
    if (c.max_qp_allowed > 63) bad = 1;
    else if (c.min_qp_allowed > 62) bad = 1;
    else if (c.min_qp_allowed > c.max_qp_allowed) bad = 1;
    if (c.tune > 2 || c.encoder_bit_depth != 8 || c.profile != 0 || c.speed_control_flag > 1) bad = 1;
    if ((int32_t)c.asm_type < 0 || (int32_t)c.asm_type > 1) bad = 1;
    if (c.target_socket != -1 && c.target_socket != 0 && c.target_socket != 1) bad = 1;
    return bad ? EB_ErrorBadParameter : EB_ErrorNone;
}

/* copy_api_from_app (:2052-2192) builds the library's copy FIRST -- hierarchical levels, frame rate from numerator / denominator, the
 * automatic intra period -- and verify_settings (:2203) judges that copy */
EbErrorType shim_resolve_config(const EbSvtVp9EncConfiguration *in, EbSvtVp9EncConfiguration *out, int *levels) {
    EbSvtVp9EncConfiguration c = *in;
    const int lv = (c.tune != 0 && c.rate_control_mode == 0) ? 4 : 3, minigop = 1 << lv;
    if (c.frame_rate_numerator != 0 && c.frame_rate_denominator != 0)
        c.frame_rate = ((c.frame_rate_numerator << 8) / c.frame_rate_denominator) << 8;
    if (c.intra_period == -2) { /* compute_default_intra_period (:2014-2024) */
        const int fps = c.frame_rate < 1000 ? (int)c.frame_rate : (int)(c.frame_rate >> 16);
        const int lo = fps / minigop * minigop, hi = (fps + minigop) / minigop * minigop;
        c.intra_period = abs(fps - hi) > abs(fps - lo) ? lo : hi;
    }
    if (verify(&c) != EB_ErrorNone) return EB_ErrorBadParameter;
    *out = c;
    *levels = lv;
    return EB_ErrorNone;
}
