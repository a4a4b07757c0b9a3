/* me_prof.h -- the marks of the ME drivers (me_sb_run, me_sb_run_fast) in the three profiling builds, decided here once:
 *   default         SVT_HIP_ME_PROFILE=1 at run time: thread 0 adds the shader cycles between marks to prof[] (general driver)
 *   -DME_FINE_PROF  the same, and the kernel ends at mark SVT_HIP_ME_STOP of list 0 (per-dispatch counters of successive launches
 *                   give cumulative counts per phase: tools/me_phase_profile.sh); fine marks inside the HME search
 *   -DME_ASM_MARKS  a comment in the assembly at every mark (static instruction counts: tools/me_static_counts.py)
 * The emulation has no clock (ME_PROF_OFF, me_prims_emu.h): every mark is a no-op. */
#ifndef SVT_ME_PROF_H
#define SVT_ME_PROF_H
#if defined(ME_PROF_OFF)
#define ME_MARK_BEGIN() ((void)0)
#define ME_MARK(i) ((void)0)
#define ME_SUBMARK_BEGIN() ((void)0)
#define ME_SUBMARK(i) ((void)0)
#define ME_STOP_AT(i) ((void)0)
#define ME_FINE_BEGIN() ((void)0)
#define ME_FINE(i) ((void)0)
#else
/* ME_MARK(i): when profiling is enabled, thread 0 adds the shader cycles since the previous mark to prof[i] */
#define ME_MARK_BEGIN() unsigned long long mark_t_ = c->prof ? __builtin_amdgcn_s_memtime() : 0
/* sub-phase marks (slots 14, 15): informational, not part of the per-phase total */
#define ME_SUBMARK_BEGIN() unsigned long long sub_t_ = c->prof ? __builtin_amdgcn_s_memtime() : 0
#define ME_SUBMARK(i) do { if (c->prof && tid == 0) { unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        atomicAdd(&c->prof[(i)], now_ - sub_t_); sub_t_ = now_; } } while (0)
#if defined(ME_ASM_MARKS)
#define ME_MARK(i) __asm__ volatile("; @MARK %0" ::"n"(i))
#define FME_MARK(i) ME_MARK(i)
#define ME_STOP_AT(i) ((void)0)
#define ME_FINE_BEGIN() ((void)0)
#define ME_FINE(i) ((void)0)
#elif defined(ME_FINE_PROF)
/* instruction-count profiling builds: the kernel stops (all threads) at mark g_me_stop_after of the first list, so
 * that per-dispatch SQ counters of successive launches give cumulative instruction counts per phase */
__device__ int g_me_stop_after = -1;
#define ME_MARK(i) do { if (c->prof && tid == 0) { unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        atomicAdd(&c->prof[(i)], now_ - mark_t_); mark_t_ = now_; } if (g_me_stop_after == (i)) return; } while (0)
#define FME_MARK(i) ME_STOP_AT(i)
#define ME_STOP_AT(i) do { if (g_me_stop_after == (i)) return; } while (0)
#define ME_FINE_BEGIN() unsigned long long ft_ = __builtin_amdgcn_s_memtime()
#define ME_FINE(i) do { if (c->prof && tid == 0) { unsigned long long n_ = __builtin_amdgcn_s_memtime(); atomicAdd(&c->prof[i], n_ - ft_); ft_ = n_; } } while (0)
#else
#define ME_MARK(i) do { if (c->prof && tid == 0) { unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        atomicAdd(&c->prof[(i)], now_ - mark_t_); mark_t_ = now_; } } while (0)
#define FME_MARK(i) ((void)0)
#define ME_STOP_AT(i) ((void)0)
#define ME_FINE_BEGIN() ((void)0)
#define ME_FINE(i) ((void)0)
#endif
#endif
#endif
