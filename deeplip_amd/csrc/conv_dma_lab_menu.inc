// Lab build only (included by conv_igemm_f16x3_dma.hip; see conv_dma_hooks.h): the stamped launch path.
#ifdef DLIP_LAB
// Lab build only (DLIP_STAMP_PRINT set): launch with the s_memtime stamps buffer, wait, print the median cycles
// between the stamps of each workgroup's first segment (tools/probes/stamps.sh).
template <typename K, typename SK>
int dlip_lab_stamped_launch(K kern, unsigned G, int threads, size_t lds, hipStream_t st, const ConvArgs& b, SK sk, int BM, int BN) {
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

// Window mode of the 256x128 tile: stride-1 convolutions with more than one tap whose output pixel m reads the input pixels
// m + const (same-size convolutions of any dilation; 1-D "valid" convolutions, where the constant grows by W - Wo per
// image), no second source, fp32 / split output; the taps' halo (+ the image shifts inside one tile) within the window's slack.
static bool win_mode_ok(const ConvArgs& a, int epi) {
  if (dlip_dbg_value[DLIP_DBG_WIN] == 0 || epi == 2 || a.x2 != nullptr) return false;
  const int taps = a.R * a.S, Ho = a.HoWo / a.Wo;
  if (a.sh != 1 || a.sw != 1 || taps < 2 || taps > 25 || (a.C & 31)) return false;
  const bool same = Ho == a.H && a.Wo == a.W;
  const bool valid1d = a.H == 1 && a.R == 1 && a.ph == 0 && a.pw == 0 && Ho == 1;
  if (!same && !valid1d) return false;
  const int D = a.H * a.W - a.HoWo;
  const int span = (a.R - 1) * a.dh * a.W + (a.S - 1) * a.dw + (D ? ((256 + a.HoWo - 1) / a.HoWo) * D : 0);
  return span <= 48 && a.ph * a.W + a.pw <= 48;
}

#endif
