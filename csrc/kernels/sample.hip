// Device-side token sampler (pra_sample): temperature / top-k / top-p draws and greedy picks from
// bf16 / fp16 logits, with the generation bookkeeping of inference.generate in the same launch.
//
// The rule (pyrecover_amd/ops/reference.py::sample_philox_ref is the same rule in torch): tokens are
// ranked by z = x / T descending, ties by ascending id, under the total order NaN < -inf < finite < +inf
// (-0 and +0 are one value). top-k keeps every token with z >= the k-th largest z; top-p keeps the
// shortest prefix of the ranking whose softmax mass (over the top-k survivors) reaches top_p; the draw is
// the first kept token whose cumulative mass exceeds u * (kept mass), the last kept one when rounding
// leaves none. u = (philox4x32_10({row, pos, 0, 3}, seed)[0] >> 8) * 2^-24: a pure function of (seed,
// row, position). A row whose maximum is not finite, and T == 0 (no Philox call), give the lowest id that
// holds the maximum.
//
// No sort. A 16-bit logit has at most 65,536 values and z is monotone in it, so the order-preserving
// 16-bit key of the logit is its rank and tokens with equal keys are exact ties. One workgroup owns a row:
//   pass 1   row maximum / minimum key and a histogram of counts over the keys: integer atomics on 16-bit
//            counters in LDS (a wave adds once for all lanes that hold its first lane's key, and once per
//            run of loads whose lanes all hold one key: an all-equal row costs one add per wave), added to
//            the 32-bit histogram in the global workspace before a counter could overflow, each bin by
//            the one thread that owns it;
//   scan     bins from the highest key down in groups of 64: per-group (count, mass) totals (thread g sums
//            group g), a block scan over the 1,024 groups, then for each of top-k / top-p / draw one lookup
//            over the group prefixes and one 64-bin wave scan inside the group that holds the threshold. mass(v) =
//            count(v) * exp2((v - vmax) * log2e / T) in fp32; every sum has a fixed association, so the
//            result is the same bits on every run, eager or replayed;
//   pass 2   the r-th token in id order whose key is the drawn one (match counts per tile of the row, a block
//            scan over the tiles, a wave scan of per-lane counts inside the tile that holds it).
// Both passes read the row 8 ids per lane at a time (one 16-B load where the row is 16-B aligned); at
// V = 128k the row is 256 KB and stays in the XCD's L2 between them.
// Integer atomics commute exactly: the histogram does not depend on arrival order.
#include "common.h"
#include "launchers.h"
#include "philox_sr.h"

namespace pra {
namespace {

constexpr int kSampleThreads = 1024;
constexpr int kSampleWaves = kSampleThreads / kWave;  // 16
constexpr int kBins = 65536;
constexpr int kGroups = kBins / kWave;  // 1024 groups of 64 bins: one per thread in the block scan
constexpr uint32_t kSampleStream = 3;   // after the stochastic-rounding streams 0, 1, 2
constexpr int kUnroll = 8;              // loads of the row a lane has in flight
constexpr int kStep = kWave * kUnroll;  // 512 ids: lane l of step `base` holds ids base + 8 l .. base + 8 l + 7
constexpr int kMaxTiles = 2048;         // tiles of a row (whole steps each) the ordered prefix count of pass 2 holds
// Pass 1 counts in LDS, two 16-bit counters per word, and adds them to the 32-bit histogram in global memory
// every kFlushRounds rounds: 7 rounds x 16 waves x 512 ids < 65,536, so no counter can overflow in between.
constexpr int kFlushRounds = 7;
static_assert(kFlushRounds * kSampleWaves * kStep < 65536, "a 16-bit LDS counter must hold a flush interval");
constexpr uint32_t kNoKey = 0xffffffffu;

static_assert(kGroups == kSampleThreads, "the block scan gives one group to each thread");

template <typename T> struct Fmt;
template <> struct Fmt<__bf16> {
  static constexpr uint32_t kInf = 0x7f80u;
  static __device__ __forceinline__ float val(uint32_t bits) { return __uint_as_float(bits << 16); }
};
template <> struct Fmt<__half> {
  static constexpr uint32_t kInf = 0x7c00u;
  static __device__ __forceinline__ float val(uint32_t bits) {
    return __half2float(__ushort_as_half((unsigned short)bits));
  }
};

// Order-preserving key of the storage bits: NaN -> 0 (below -inf), +-0 -> 0x8000.
template <typename T>
__device__ __forceinline__ uint32_t key_of(uint32_t h) {
  const uint32_t a = h & 0x7fffu;
  if (a > Fmt<T>::kInf) return 0u;
  if (a == 0u) return 0x8000u;
  return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}
template <typename T>
__device__ __forceinline__ float val_of_key(uint32_t key) {
  return Fmt<T>::val((key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu));
}
template <typename T>
__device__ __forceinline__ bool key_finite(uint32_t key) {
  return key > ((~(0x8000u | Fmt<T>::kInf)) & 0xffffu) && key < (0x8000u | Fmt<T>::kInf);
}

// The keys of one step of the row: lane l holds ids base + 8 l .. base + 8 l + 7 (key[j]: id base + 8 l + j),
// ids >= V give kNoKey. A whole step of a 16-B aligned row is one 16-B load per lane; otherwise eight
// 2-B loads, all issued before the first use.
template <typename T>
__device__ __forceinline__ void load_step(const uint16_t* __restrict__ x, int base, int V, int lane, bool vec,
                                          uint32_t (&key)[kUnroll]) {
  const int i0 = base + lane * kUnroll;
  if (vec && base + kStep <= V) {  // wave-uniform
    const uint4 q = *reinterpret_cast<const uint4*>(x + i0);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      key[2 * j] = key_of<T>(w[j] & 0xffffu);
      key[2 * j + 1] = key_of<T>(w[j] >> 16);
    }
  } else {
    uint16_t raw[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) raw[j] = i0 + j < V ? x[i0 + j] : (uint16_t)0;
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) key[j] = i0 + j < V ? key_of<T>(raw[j]) : kNoKey;
  }
}

__device__ __forceinline__ float wave_incl_scan(float v, int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const float t = __shfl_up(v, o, kWave);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v, int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const unsigned t = __shfl_up(v, o, kWave);
    if (lane >= o) v += t;
  }
  return v;
}

// The lane's bin of group g (position q = 64 g + lane in the ranking of keys, key = 65535 - q) and the
// exclusive prefixes of count and mass inside the group. The histogram was stored by other waves of the
// block: it is read with agent-scope loads, which do not hit a stale line of this CU's L1.
struct Bin {
  unsigned cnt, exc;
  float e, mass, exm;
};
template <typename T>
__device__ __forceinline__ Bin load_group(const unsigned* hist, int g, int lane, float vmax, float c) {
  const uint32_t key = 65535u - (uint32_t)(g * kWave + lane);
  Bin b;
  b.cnt = __hip_atomic_load(hist + key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  b.e = 0.f;
  if (b.cnt != 0u && key != 0u) b.e = exp2f((val_of_key<T>(key) - vmax) * c);  // NaN bin: no mass
  b.mass = (float)b.cnt * b.e;
  const float im = wave_incl_scan(b.mass, lane);
  const unsigned ic = wave_incl_scan(b.cnt, lane);
  const float pm = __shfl_up(im, 1, kWave);
  const unsigned pc = __shfl_up(ic, 1, kWave);
  b.exm = lane ? pm : 0.f;
  b.exc = lane ? pc : 0u;
  return b;
}

struct SampleParams {
  pra_sample_args a;
  float c;  // log2(e) / temperature
};

template <typename T>
__global__ __launch_bounds__(kSampleThreads) void sample_kernel(const T* __restrict__ logits, long ld, int V,
                                                                SampleParams p) {
  __shared__ unsigned Gc[kGroups], Pc[kGroups + 1];
  __shared__ float Gm[kGroups], Pm[kGroups + 1];
  __shared__ unsigned wsc[kSampleWaves];
  __shared__ float wsm[kSampleWaves];
  __shared__ unsigned s_kmax[kSampleWaves], s_kmin[kSampleWaves];
  __shared__ unsigned tile_cnt[kMaxTiles];
  __shared__ unsigned lds_hist[kBins / 2];  // bin 2 w in the low half of word w, bin 2 w + 1 in the high half
  __shared__ int s_sel[3];
  __shared__ int s_tok;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.x;
  const pra_sample_args& a = p.a;
  const pra_sample_state& gs = a.gen;
  const bool stateful = gs.done != nullptr;
  if (stateful && gs.done[b]) {  // block-uniform: a finished row writes nothing but its (zero) next input
    if (tid == 0) a.tok[b] = 0;
    return;
  }
  const int cur = stateful ? gs.count[b] : 0;
  const bool greedy = !(a.temperature > 0.f);
  float u = 0.f;
  if (!greedy) {
    const int pos = gs.prompt_len != nullptr ? gs.prompt_len[b] + cur : a.pos[b];
    uint32_t rnd[4];
    philox4x32_10((uint32_t)b, (uint32_t)pos, 0u, kSampleStream, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), rnd);
    u = (float)(rnd[0] >> 8) * 0x1p-24f;
    if (tid == 0 && a.u_out != nullptr) a.u_out[b] = u;
  }
  const uint16_t* x = reinterpret_cast<const uint16_t*>(logits) + (long)b * ld;
  unsigned* hist = a.ws + (long)b * kBins;
  const bool vec = reinterpret_cast<uintptr_t>(x) % 16 == 0;

  if (tid == 0) {
    s_sel[0] = 0;
    s_sel[1] = -1;
    s_sel[2] = kGroups;
    s_tok = -1;
  }
  if (!greedy)
    for (int w = tid; w < kBins / 2; w += kSampleThreads) lds_hist[w] = 0u;
  __syncthreads();

  // ---- pass 1: step s of the row (512 ids) goes to wave s % 16 in round s / 16
  const int tile_steps = (V + kStep * kMaxTiles - 1) / (kStep * kMaxTiles);  // 1 up to V = 2^20
  const int tile_elems = tile_steps * kStep;
  const int ntiles = (V + tile_elems - 1) / tile_elems;
  {
    const auto count = [&](uint32_t key, unsigned n) { atomicAdd(&lds_hist[key >> 1], n << ((key & 1u) * 16u)); };
    uint32_t kmax = 0u, kmin = 0xffffu;
    uint32_t run_key = 0u;
    unsigned run_cnt = 0u;  // wave-uniform: a run of (step, j) whose lanes all held run_key
    const int nrounds = ((V + kStep - 1) / kStep + kSampleWaves - 1) / kSampleWaves;
    for (int rd = 0; rd < nrounds; ++rd) {
      const int base = (rd * kSampleWaves + wid) * kStep;
      if (base < V) {
        uint32_t keys[kUnroll];
        load_step<T>(x, base, V, lane, vec, keys);
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) {
          const uint32_t key = keys[j];
          bool pend = key != kNoKey;
          if (pend) {
            kmax = max(kmax, key);
            kmin = min(kmin, key);
          }
          const unsigned long long mv = __ballot(pend);
          if (greedy || mv == 0ull) continue;
          const int leader = __ffsll((long long)mv) - 1;
          const uint32_t lk = __builtin_amdgcn_readlane(key, leader);
          const bool same = pend && key == lk;
          const unsigned long long sm = __ballot(same);
          if (sm == mv) {  // every lane holds lk: extend the run
            if (run_cnt != 0u && lk != run_key) {
              if (lane == 0) count(run_key, run_cnt);
              run_cnt = 0u;
            }
            run_key = lk;
            run_cnt += (unsigned)__popcll(mv);
            continue;
          }
          if (lane == leader) count(lk, (unsigned)__popcll(sm));  // one add for the first lane's key ...
          if (pend && !same) count(key, 1u);                       // ... and one per lane for the rest
        }
      }
      if (!greedy && ((rd + 1) % kFlushRounds == 0 || rd + 1 == nrounds)) {  // block-uniform
        if (run_cnt != 0u && lane == 0) count(run_key, run_cnt);
        run_cnt = 0u;
        __syncthreads();
        // thread t owns words t, t + 1024, ...: the first flush stores every bin (the workspace may hold
        // anything), later ones add; no other thread touches these bins in global memory
        uint2* h2 = reinterpret_cast<uint2*>(hist);
        for (int w = tid; w < kBins / 2; w += kSampleThreads) {
          const unsigned v = lds_hist[w];
          if (rd < kFlushRounds) {
            h2[w] = make_uint2(v & 0xffffu, v >> 16);
          } else if (v != 0u) {
            uint2 o = h2[w];
            o.x += v & 0xffffu;
            o.y += v >> 16;
            h2[w] = o;
          }
          if (v != 0u) lds_hist[w] = 0u;
        }
        __syncthreads();
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      kmax = max(kmax, (uint32_t)__shfl_xor(kmax, o, kWave));
      kmin = min(kmin, (uint32_t)__shfl_xor(kmin, o, kWave));
    }
    if (lane == 0) {
      s_kmax[wid] = kmax;
      s_kmin[wid] = kmin;
    }
  }
  if (!greedy) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's histogram stores are performed ...
  }
  __syncthreads();
  if (!greedy) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // ... and this CU's L1 holds no older copy
  uint32_t kmax = 0u, kmin = 0xffffu;
#pragma unroll
  for (int w = 0; w < kSampleWaves; ++w) {
    kmax = max(kmax, s_kmax[w]);
    kmin = min(kmin, s_kmin[w]);
  }

  uint32_t kd = kmax;  // the drawn key, and the index r among its tokens in id order
  int r = 0;
  if (!greedy && key_finite<T>(kmax)) {  // block-uniform
    const float vmax = val_of_key<T>(kmax);
    // ---- group totals: thread g sums the 64 bins of group g from the highest key down (256 contiguous
    // bytes, all loads in flight at once), then the block scan over the groups
    {
      const uint32_t key0 = (uint32_t)(kBins - kWave) - (uint32_t)tid * kWave;  // the group's lowest key
      const uint4* src = reinterpret_cast<const uint4*>(hist + key0);
      uint4 v[kWave / 4];
#pragma unroll
      for (int i = 0; i < kWave / 4; ++i) v[i] = src[i];
      unsigned gc = 0u;
      float gm = 0.f;
#pragma unroll
      for (int i = kWave - 1; i >= 0; --i) {
        const uint4 q = v[i >> 2];
        const unsigned cnt = (i & 3) == 0 ? q.x : (i & 3) == 1 ? q.y : (i & 3) == 2 ? q.z : q.w;
        const uint32_t key = key0 + (uint32_t)i;
        if (cnt != 0u) {
          gc += cnt;
          if (key != 0u) gm += (float)cnt * exp2f((val_of_key<T>(key) - vmax) * p.c);
        }
      }
      Gc[tid] = gc;
      Gm[tid] = gm;
    }
    __syncthreads();
    {
      const unsigned ic = wave_incl_scan(Gc[tid], lane);
      const float im = wave_incl_scan(Gm[tid], lane);
      if (lane == kWave - 1) {
        wsc[wid] = ic;
        wsm[wid] = im;
      }
      const unsigned pc = __shfl_up(ic, 1, kWave);
      const float pm = __shfl_up(im, 1, kWave);
      __syncthreads();
      unsigned oc = 0u;
      float om = 0.f;
      for (int w = 0; w < wid; ++w) {
        oc += wsc[w];
        om += wsm[w];
      }
      Pc[tid] = oc + (lane ? pc : 0u);
      Pm[tid] = om + (lane ? pm : 0.f);
      if (tid == kSampleThreads - 1) {
        Pc[kGroups] = oc + ic;
        Pm[kGroups] = om + im;
      }
    }
    __syncthreads();

    // ---- top-k: the last kept position qk of the key ranking, and the mass Zk down to it
    const bool use_k = a.top_k > 0 && a.top_k < V;
    const unsigned k = (unsigned)a.top_k;
    if (use_k && Pc[tid] < k && k <= Pc[tid] + Gc[tid]) s_sel[0] = tid;  // exactly one group
    __syncthreads();
    int qk;
    float Zk;
    unsigned cnt_k;
    {
      int g, l;
      if (use_k) {
        g = s_sel[0];
      } else {
        g = (int)(65535u - kmin) >> 6;
      }
      const Bin bn = load_group<T>(hist, g, lane, vmax, p.c);
      if (use_k) {
        const unsigned before = Pc[g] + bn.exc;
        const unsigned long long m = __ballot(bn.cnt != 0u && before < k && k <= before + bn.cnt);
        l = m ? __ffsll((long long)m) - 1 : 0;
      } else {
        l = (int)(65535u - kmin) & 63;
      }
      qk = g * kWave + l;
      Zk = __shfl((Pm[g] + bn.exm) + bn.mass, l, kWave);
      cnt_k = __shfl(bn.cnt, l, kWave);
    }

    // ---- top-p: the last kept position qp, how many of its ties stay (np), the kept mass
    int qp = qk;
    unsigned np = cnt_k;
    float Zkept = Zk;
    if (a.top_p < 1.f) {
      const float pz = a.top_p * Zk;
      if (tid <= (qk >> 6) && Gc[tid] != 0u && Pm[tid] < pz) atomicMax(&s_sel[1], tid);
      __syncthreads();
      const int g = max(s_sel[1], 0);
      const Bin bn = load_group<T>(hist, g, lane, vmax, p.c);
      const int q = g * kWave + lane;
      const float before = Pm[g] + bn.exm;
      const unsigned long long m = __ballot(bn.cnt != 0u && q <= qk && before < pz);
      if (m != 0ull) {  // always: the group's first bin has before == Pm[g]
        const int l = 63 - __clzll((long long)m);
        const float bl = __shfl(before, l, kWave), el = __shfl(bn.e, l, kWave);
        const unsigned cl = __shfl(bn.cnt, l, kWave);
        const float nf = ceilf((pz - bl) / el);
        np = !(nf >= 1.f) ? 1u : (nf >= (float)cl ? cl : (unsigned)nf);
        qp = g * kWave + l;
        Zkept = bl + (float)np * el;
      }
    }

    // ---- draw: the first kept position whose cumulative kept mass exceeds u * Zkept
    const float target = u * Zkept;
    {
      const int gp = qp >> 6;
      if (tid <= gp && Gc[tid] != 0u && (tid == gp || Pm[tid + 1] > target)) atomicMin(&s_sel[2], tid);
      __syncthreads();
      const int g = min(s_sel[2], gp);
      const Bin bn = load_group<T>(hist, g, lane, vmax, p.c);
      const int q = g * kWave + lane;
      const float before = Pm[g] + bn.exm;
      const unsigned effc = q == qp ? np : bn.cnt;
      const bool elig = bn.cnt != 0u && q <= qp;
      const unsigned long long me = __ballot(elig);
      const unsigned long long mh = __ballot(elig && before + (float)effc * bn.e > target);
      int l;
      if (mh != 0ull) {
        l = __ffsll((long long)mh) - 1;
        const float rf = floorf((target - __shfl(before, l, kWave)) / __shfl(bn.e, l, kWave));
        const unsigned cl = __shfl(effc, l, kWave);
        r = !(rf >= 0.f) ? 0 : (rf >= (float)cl ? (int)cl - 1 : (int)rf);
      } else {  // rounding left none: the last kept token of this group
        l = me ? 63 - __clzll((long long)me) : 0;
        r = (int)__shfl(effc, l, kWave) - 1;
      }
      kd = 65535u - (uint32_t)(g * kWave + l);
      if (r < 0) r = 0;
    }
  }

  // ---- pass 2: the r-th id, ascending, whose key is kd: matches per tile, a block scan over the tiles,
  // then one wave walks the tile that holds it
  {
    for (int t = wid; t < ntiles; t += kSampleWaves) {
      unsigned n = 0u;
      for (int st = 0; st < tile_steps; ++st) {
        const int base = t * tile_elems + st * kStep;
        if (base >= V) break;
        uint32_t keys[kUnroll];
        load_step<T>(x, base, V, lane, vec, keys);
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) n += keys[j] == kd ? 1u : 0u;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) n += (unsigned)__shfl_xor(n, o, kWave);
      if (lane == 0) tile_cnt[t] = n;
    }
    __syncthreads();
    constexpr int kPer = kMaxTiles / kSampleThreads;  // tiles per thread
    unsigned c[kPer], local = 0u;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int t = tid * kPer + i;
      c[i] = t < ntiles ? tile_cnt[t] : 0u;
      local += c[i];
    }
    const unsigned incl = wave_incl_scan(local, lane);
    if (lane == kWave - 1) wsc[wid] = incl;
    __syncthreads();
    unsigned total = 0u, off = 0u;
    for (int w = 0; w < kSampleWaves; ++w) {
      if (w == wid) off = total;
      total += wsc[w];
    }
    unsigned want = (unsigned)r;
    if (total != 0u && want >= total) want = total - 1u;
    unsigned before = off + incl - local;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      if (want >= before && want < before + c[i]) {  // exactly one (thread, i) when total > 0
        s_sel[0] = tid * kPer + i;
        s_sel[1] = (int)before;
      }
      before += c[i];
    }
    __syncthreads();
    if (wid == 0 && total != 0u) {
      const int t = s_sel[0];
      unsigned seen = (unsigned)s_sel[1];
      bool found = false;
      for (int st = 0; st < tile_steps && !found; ++st) {
        const int base = t * tile_elems + st * kStep;
        if (base >= V) break;
        uint32_t keys[kUnroll];
        load_step<T>(x, base, V, lane, vec, keys);
        unsigned c = 0u;
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) c += keys[j] == kd ? 1u : 0u;
        const unsigned incl = wave_incl_scan(c, lane);  // ids ascend with the lane, then with j
        const unsigned tot = __shfl(incl, kWave - 1, kWave);
        if (want < seen + tot) {
          const unsigned lo = seen + incl - c;
          if (want >= lo && want < lo + c) {  // one lane
            int k = (int)(want - lo);
#pragma unroll
            for (int j = 0; j < kUnroll; ++j)
              if (keys[j] == kd) {
                if (k == 0) s_tok = base + lane * kUnroll + j;
                --k;
              }
          }
          found = true;
        }
        seen += tot;
      }
    }
    __syncthreads();
  }

  if (tid == 0) {
    long long tok = s_tok < 0 ? 0 : s_tok;
    if (stateful) {
      bool fin = false;
      if (cur >= 0 && cur < gs.max_new) {
        gs.out[(long)b * gs.max_new + cur] = tok;
        gs.count[b] = cur + 1;
        fin = tok == gs.eos_id || cur + 1 > gs.room[b];  // token `room` is the last one with a cache row before it
      } else {
        fin = true;
      }
      if (fin) {
        gs.done[b] = 1;
        tok = 0;  // the next decode step's input of a finished row
      }
    }
    a.tok[b] = tok;
  }
}

}  // namespace
}  // namespace pra

extern "C" {

long pra_sample_ws_bytes(int B) { return B > 0 ? (long)B * pra::kBins * (long)sizeof(unsigned) : 0; }

hipError_t pra_sample(int dtype, const void* logits, long ld, int B, int V, const pra_sample_args* args,
                      hipStream_t s) {
  if (args == nullptr || logits == nullptr || B <= 0 || B > 65535 || V <= 0 || V > (1 << 30) || ld < V || args->tok == nullptr)
    return hipErrorInvalidValue;
  const bool greedy = !(args->temperature > 0.f);
  if (args->temperature < 0.f || args->top_k < 0 || !(args->top_p > 0.f && args->top_p <= 1.f))
    return hipErrorInvalidValue;
  if (!greedy && (args->ws == nullptr || reinterpret_cast<uintptr_t>(args->ws) % 16 != 0 || (args->pos == nullptr && args->gen.prompt_len == nullptr)))
    return hipErrorInvalidValue;
  const pra_sample_state& g = args->gen;
  if (g.done != nullptr && (g.count == nullptr || g.room == nullptr || g.out == nullptr || g.max_new <= 0))
    return hipErrorInvalidValue;
  if (g.done == nullptr && g.prompt_len != nullptr) return hipErrorInvalidValue;
  pra::SampleParams p;
  p.a = *args;
  p.c = greedy ? 0.f : (float)(1.4426950408889634 / (double)args->temperature);
  PRA_DISPATCH_16BIT(dtype, T, {
    hipLaunchKernelGGL(pra::sample_kernel<T>, dim3(B), dim3(pra::kSampleThreads), 0, s, (const T*)logits, ld, V, p);
    return hipGetLastError();
  });
  return hipErrorInvalidValue;
}
}
