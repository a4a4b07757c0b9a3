/*
 * coef_update_emu.cpp -- csrc/coef_update.hip itself (kernels and entry point, included below) on the CPU through the stand-in runtime of
 * tests/emu/hip/hip_runtime.h, compared with svt_hip_coef_update_picture: batches of pictures with unlike stream lengths (empty, one
 * record, the count kernel's pass and grid-stride boundaries), totals on the "device" and in the descriptor, with and without "old"
 * tables of their own.  Every buffer is allocated to exactly its size: the sanitizers see a record read or written one past an end.
 * argv[1]: a file holding one svt_bool_tables.
 */
#include <hip/hip_runtime.h>
inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#include "coef_update.hip"
#include "emu_harness.h"
#include <random>
#include <memory>

static std::vector<uint32_t> stream(std::mt19937 &rng, uint32_t n, int shape) {
    std::vector<uint32_t> t(n);
    int                   c = 0, grp = 0, prev = -1;
    for (uint32_t i = 0; i < n; i++) {
        if (c == 0) grp = shape == 2 ? 4 + (int)(rng() % 4) : (int)(rng() % 16);
        int tok = shape == 1 ? (rng() % 100 < 75 ? 0 : rng() % 100 < 60 ? 11 : 1) : rng() % 100 < 45 ? 0 : rng() % 100 < 40 ? 1 : rng() % 100 < 30 ? 11 : 2 + (int)(rng() % 9);
        if (tok == 11 && prev == 0) tok = 1;
        if ((c >= 30 || i + 1 == n) && tok == 0) tok = 2;
        const int band = c == 0 ? 0 : c < 3 ? 1 : c < 6 ? 2 : c < 10 ? 3 : c < 21 ? 4 : 5, ctx6 = band ? rng() % 6 : rng() % 3;
        t[i] = SVT_TOK_RECORD(tok && tok != 11 ? rng() & 0xffff : 0, (grp * 6 + band) * 6 + ctx6, tok);
        prev = tok;
        c = tok == 11 || c >= 30 ? 0 : c + 1;
        if (c == 0) prev = -1;
    }
    return t;
}

struct pic_buffers {
    std::unique_ptr<uint32_t[]> tok, ntok, counts, eob, n;
    std::unique_ptr<uint8_t[]>  old, probs;
    std::unique_ptr<uint16_t[]> bools;
    std::unique_ptr<svt_bool_segment[]> seg;
    std::unique_ptr<svt_cu_result[]>    res;
    svt_cu_picture p;
    pic_buffers(const std::vector<uint32_t> &t, bool dev_count, bool own_old, std::mt19937 &rng, const pic_buffers *like)
        : tok(new uint32_t[t.size()]), ntok(new uint32_t[1]), counts(new uint32_t[SVT_TOK_COUNTS]), eob(new uint32_t[SVT_CU_ROWS]), n(new uint32_t[1]),
          old(new uint8_t[SVT_CU_PROBS]), probs(new uint8_t[SVT_CU_PROBS]), bools(new uint16_t[svt_hip_coef_update_bools_capacity()]), seg(new svt_bool_segment[1]),
          res(new svt_cu_result[1]) {
        memset(&p, 0, sizeof p);
        memset(counts.get(), 0, sizeof(uint32_t) * SVT_TOK_COUNTS);
        for (size_t i = 0; i < t.size(); i++) { tok[i] = t[i]; counts[SVT_TOK_PROB_ROW(t[i]) * 12 + SVT_TOK_TOKEN(t[i])]++; }
        if (like) memcpy(old.get(), like->old.get(), SVT_CU_PROBS);
        else for (int i = 0; i < SVT_CU_PROBS; i++) old[i] = (uint8_t)(rng() % 23 == 0 ? (rng() & 1 ? 1 : 255) : 1 + rng() % 255);
        memset(res.get(), 0xEE, sizeof(svt_cu_result));
        ntok[0] = (uint32_t)t.size();
        p.d_tokens = t.empty() ? nullptr : tok.get();
        p.d_n_tokens = dev_count ? ntok.get() : nullptr;
        p.n_tokens = dev_count ? 0 : (uint32_t)t.size();
        p.max_tokens = (uint32_t)t.size();
        p.d_counts = counts.get(); p.d_old_probs = own_old ? old.get() : nullptr;
        p.d_eob_branch = eob.get(); p.d_probs = probs.get(); p.d_hdr_bools = bools.get(); p.d_n_hdr_bools = n.get(); p.d_segment = seg.get(); p.d_result = res.get();
        if (like) { p.n_prefix = like->p.n_prefix; p.n_suffix = like->p.n_suffix; memcpy(p.prefix, like->p.prefix, sizeof p.prefix); memcpy(p.suffix, like->p.suffix, sizeof p.suffix); }
        else {
            p.n_prefix = (uint16_t)(rng() % (SVT_CU_PREFIX_MAX + 1)); p.n_suffix = (uint16_t)(rng() % (SVT_CU_SUFFIX_MAX + 1));
            for (int i = 0; i < p.n_prefix; i++) p.prefix[i] = SVT_BOOL_RECORD(rng() & 1, 128);
            for (int i = 0; i < p.n_suffix; i++) p.suffix[i] = SVT_BOOL_RECORD(0, 252);
        }
    }
};

int main(int argc, char **argv) {
    static svt_hip_ctx ctx;
    svt_bool_tables    tab;
    FILE              *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f || fread(&tab, sizeof tab, 1, f) != 1) return 2;
    ctx.slot[SVT_SLOT_BC_TABLES] = &tab; ctx.slot_bytes[SVT_SLOT_BC_TABLES] = sizeof tab;
    std::mt19937 rng(7);
    int          bad = 0;
    const uint32_t pass = CU_ITEMS, wrap = CU_ITEMS * CU_MAX_WGS;
    /* batches: lengths around the pass and the grid-stride boundaries, then unlike lengths with and without tables of their own */
    const std::vector<std::vector<uint32_t>> batches = {{0, 1, pass - 1, pass, pass + 1, 2 * pass + 5}, {wrap - 1, wrap, wrap + 1}, {300, 9000, 25, 70001, 0, 4097}};
    for (size_t b = 0; b < batches.size(); b++) {
        std::vector<std::unique_ptr<pic_buffers>> dev, host;
        std::vector<svt_cu_picture>               pics;
        for (size_t i = 0; i < batches[b].size(); i++) {
            const std::vector<uint32_t> t = stream(rng, batches[b][i], b == 1 ? 1 : (int)(i % 3));
            const bool own = b != 0 && (i % 3) != 2; /* the others are measured against the context's table */
            dev.emplace_back(new pic_buffers(t, i & 1, own, rng, nullptr));
            host.emplace_back(new pic_buffers(t, i & 1, own, rng, dev.back().get()));
            pics.push_back(dev.back()->p);
        }
        const int rc = svt_hip_coef_update_batch_device(&ctx, (int)pics.size(), pics.data());
        for (size_t i = 0; i < pics.size(); i++) {
            const int  rh = svt_hip_coef_update_picture(&host[i]->p, &tab);
            const bool ok = !rc && !rh && dev[i]->n[0] == host[i]->n[0] && !memcmp(dev[i]->bools.get(), host[i]->bools.get(), sizeof(uint16_t) * host[i]->n[0]) &&
                            !memcmp(dev[i]->eob.get(), host[i]->eob.get(), sizeof(uint32_t) * SVT_CU_ROWS) && !memcmp(dev[i]->probs.get(), host[i]->probs.get(), SVT_CU_PROBS) &&
                            !memcmp(dev[i]->res.get(), host[i]->res.get(), sizeof(svt_cu_result)) && !memcmp(dev[i]->seg.get(), host[i]->seg.get(), sizeof(svt_bool_segment));
            printf("batch %zu picture %zu tokens %u bools %u updated %u %u %u %u sent %u%u%u%u %s\n", b, i, batches[b][i], host[i]->n[0], host[i]->res[0].updated[0],
                   host[i]->res[0].updated[1], host[i]->res[0].updated[2], host[i]->res[0].updated[3], host[i]->res[0].sent[0], host[i]->res[0].sent[1], host[i]->res[0].sent[2],
                   host[i]->res[0].sent[3], ok ? "ok" : "MISMATCH");
            bad += !ok;
        }
    }
    /* refusals launch nothing */
    svt_cu_picture none;
    memset(&none, 0, sizeof none);
    bad += svt_hip_coef_update_batch_device(&ctx, 1, &none) == 0;
    bad += svt_hip_coef_update_batch_device(&ctx, 0, &none) == 0;
    bad += svt_hip_coef_update_batch_device(&ctx, 1, nullptr) == 0;
    printf("bad %d\n", bad);
    return bad;
}
