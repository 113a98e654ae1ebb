// In-kernel stamps of the LDS-DMA ring kernel (conv_igemm_f16x3_dma.hip).  `python -m deeplip_amd.build --lab` (-DDLIP_LAB:
// libdeeplip_hip_lab.so, used by tools/ through DLIP_LIB_PATH, never by the product) compiles the PRODUCT kernels with time stamps
// and a stamped launch path; the product build gets the empty column of this table.  The kernel's text carries no #ifdef: it
// names these macros where a stamp is taken.
//
//   macro                             product      lab build
//   DLIP_LAB_STREAMK_FIELDS           (nothing)    unsigned long long* stamps
//   DLIP_STAMP / SSTAMP / BSTAMP      (nothing)    s_memtime of thread 0 (wave 4 for BSTAMP) into sk.stamps
//   DLIP_LAB_WG_STAMP(slot, c)        (nothing)    s_memrealtime into slot `slot` under condition c
//   DLIP_LAB_SEGMENT_END_STAMPS()     (nothing)    the closing stamps of a workgroup's first segment ...
//   DLIP_LAB_WG_END_STAMPS()          (nothing)    ... and of the workgroup
//   DLIP_LAB_LAUNCH_HOOK()            (nothing)    DLIP_STAMP_PRINT set: dlip_lab_stamped_launch (below) instead of the plain launch
#pragma once
#ifdef DLIP_LAB
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define DLIP_LAB_STREAMK_FIELDS unsigned long long* stamps;   /* [G][10] s_memtime values of each workgroup's first segment */
#define DLIP_STAMP(i) do { if (threadIdx.x == 0 && it == it_begin && sk.stamps) sk.stamps[(size_t)g * 10 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
// inside ONE slice (the 9th of each workgroup's first segment): [(G + g) * 10 + i]
#define DLIP_SSTAMP(i) do { if (threadIdx.x == 0 && it == it_begin && kt == 8 && sk.stamps) sk.stamps[((size_t)sk.G + g) * 10 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
// the same slice as seen by wave 4 (the ping-pong loop's half B): [(2 G + g) * 10 + i]
#define DLIP_BSTAMP(i) do { if (threadIdx.x == 256 && it == it_begin && kt == 8 && sk.stamps) sk.stamps[((size_t)2 * sk.G + g) * 10 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#define DLIP_LAB_WG_STAMP(slot, cond) do { if (threadIdx.x == 0 && (cond) && sk.stamps) sk.stamps[(size_t)g * 10 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define DLIP_LAB_SEGMENT_END_STAMPS() do { \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
    if (threadIdx.x == 0 && it == it_begin && sk.stamps) { \
      sk.stamps[(size_t)g * 10 + 5] = __builtin_amdgcn_s_memtime(); \
      sk.stamps[(size_t)g * 10 + 6] = (unsigned long long)kn; \
      sk.stamps[(size_t)g * 10 + 7] = __builtin_amdgcn_s_memrealtime() - sk.stamps[(size_t)g * 10 + 7]; \
    } } while (0)
#define DLIP_LAB_WG_END_STAMPS() do { \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
    if (threadIdx.x == 0 && sk.stamps) { \
      sk.stamps[(size_t)g * 10 + 9] = __builtin_amdgcn_s_memrealtime(); \
      sk.stamps[(size_t)g * 10 + 6] |= (unsigned long long)(blockIdx.x & 7) << 32; \
    } } while (0)
// host side (launch_one of conv_igemm_f16x3_dma.hip)
#define DLIP_LAB_LAUNCH_HOOK() do { sk.stamps = nullptr; \
    if (getenv("DLIP_STAMP_PRINT")) { if (!getenv("DLIP_STAMP_REDUCE_LATER")) sk.reduce_later = 0;   /* (stamped launches skip the reduce launch) */ \
      return dlip_lab_stamped_launch(kern, (unsigned)G, threads, lds, st, b, sk, BM, BN); } } while (0)

// DLIP_STAMP_PRINT set: launch with the s_memtime stamps buffer, wait, print the median cycles between the stamps of each
// workgroup's first segment (tools/probes/stamps.sh).
template <typename K, typename SK>
static int dlip_lab_stamped_launch(K kern, unsigned G, int threads, size_t lds, hipStream_t st, const ConvArgs& b, SK sk, int BM, int BN) {
  static unsigned long long* dbuf = nullptr;
  static size_t cap = 0;
  if (cap < (size_t)G * 30) { if (dbuf) (void)hipFree(dbuf); (void)hipMalloc(reinterpret_cast<void**>(&dbuf), (size_t)G * 30 * 8); cap = (size_t)G * 30; }
  (void)hipMemsetAsync(dbuf, 0, (size_t)G * 30 * 8, st);
  sk.stamps = dbuf;
  hipLaunchKernelGGL(kern, dim3(G), dim3(threads), lds, st, b, sk);
  (void)hipStreamSynchronize(st);
  std::vector<unsigned long long> h((size_t)G * 30);
  (void)hipMemcpy(h.data(), dbuf, h.size() * 8, hipMemcpyDeviceToHost);
  std::vector<double> d[5], per, clk, dur;
  unsigned long long t0 = ~0ull, t1 = 0, s1 = 0;
  for (unsigned i = 0; i < G; ++i) {
    const unsigned long long* r = &h[(size_t)i * 10];
    if (r[5]) {
      for (int j = 0; j < 5; ++j) d[j].push_back((double)(r[j + 1] - r[j]));
      per.push_back((double)(r[4] - r[3]) / (double)((r[6] & 0xffffffffull) ? (r[6] & 0xffffffffull) : 1));
      if (r[7]) clk.push_back((double)(r[5] - r[0]) / (double)r[7] * 100.0);   // MHz: s_memtime ticks per 100 MHz s_memrealtime tick
    }
    if (r[9]) {
      t0 = r[8] < t0 ? r[8] : t0; s1 = r[8] > s1 ? r[8] : s1; t1 = r[9] > t1 ? r[9] : t1;
      dur.push_back((double)(r[9] - r[8]) / 100.0);
    }
  }
  auto med = [](std::vector<double>& v) { if (v.empty()) return 0.0; std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
  std::sort(dur.begin(), dur.end());
  if (!dur.empty())
    fprintf(stderr, "[stamps wall] kernel span %.1f us; workgroup starts spread %.1f us; workgroup busy min %.1f med %.1f max %.1f us\n",
            (double)(t1 - t0) / 100.0, (double)(s1 - t0) / 100.0, dur.front(), dur[dur.size() / 2], dur.back());
  fprintf(stderr, "[stamps %dx%d M=%d K=%d nk=%d G=%u] setup %.0f  issue+init %.0f  first-wait %.0f  loop %.0f (%.0f/slice)  tail %.0f  clock %.0f MHz\n",
          BM, BN, b.M, b.K, b.nk, G, med(d[0]), med(d[1]), med(d[2]), med(d[3]), med(per), med(d[4]), med(clk));
  std::vector<double> e[6];
  for (unsigned i = 0; i < G; ++i) {
    const unsigned long long* r = &h[((size_t)G + i) * 10];
    if (r[6] && r[0]) for (int j = 0; j < 6; ++j) e[j].push_back((double)(r[j + 1] - r[j]));
  }
  fprintf(stderr, "[slice 8 of the first segment, wave 0] piece issue %.0f  rest reads + group 0 %.0f  group 1 + half of 2 %.0f  vmcnt wait %.0f  barrier %.0f  first reads + rest of group 2 %.0f\n",
          med(e[0]), med(e[1]), med(e[2]), med(e[3]), med(e[4]), med(e[5]));
  {   // ping-pong loop: the same slice in half B (wave 4); for half A the line above reads: LOAD | barrier | matrix phase | - | barrier | wait
    std::vector<double> f[5];
    for (unsigned i = 0; i < G; ++i) {
      const unsigned long long* r = &h[((size_t)2 * G + i) * 10];
      if (r[5] && r[0]) for (int j = 0; j < 5; ++j) f[j].push_back((double)(r[j + 1] - r[j]));
    }
    if (!f[0].empty())
      fprintf(stderr, "[ping-pong, the same slice in half B (wave 4)] LOAD %.0f  vmcnt wait %.0f  barrier %.0f  matrix phase %.0f  barrier %.0f\n",
              med(f[0]), med(f[1]), med(f[2]), med(f[3]), med(f[4]));
  }
  return dlip_launch_status();
}
#else
#define DLIP_LAB_STREAMK_FIELDS
#define DLIP_STAMP(i) do { } while (0)
#define DLIP_SSTAMP(i) do { } while (0)
#define DLIP_BSTAMP(i) do { } while (0)
#define DLIP_LAB_WG_STAMP(slot, cond) do { } while (0)
#define DLIP_LAB_SEGMENT_END_STAMPS() do { } while (0)
#define DLIP_LAB_WG_END_STAMPS() do { } while (0)
#define DLIP_LAB_LAUNCH_HOOK() do { } while (0)
#endif
