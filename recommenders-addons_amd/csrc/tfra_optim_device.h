// Optimizer update rules shared by the fused write-back kernels (tfra_optim.hip,
// tfra_apply_device.h), and the kernels' parameter records OptP / ScoreP (formed on the host by opt_of / score_of, tfra_host.h).  TF's ResourceApply{GradientDescent,Adam,Adagrad[V2],Ftrl,Momentum,RMSProp}, fp32, same
// operation order as oracle/optimizers.py; compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <type_traits>

#include "../../include/tfra_mi355x.h"

namespace tfra {

struct OptP {
  int kind;
  float lr, beta1, beta2, eps, l1, l2, lr_power;
  const float* d_lr;  // optional device scalar overriding lr
};

__device__ __forceinline__ float sgnf(float z) { return (z > 0.f) ? 1.f : ((z < 0.f) ? -1.f : 0.f); }

template <int KIND>
__device__ __forceinline__ void apply_one(const OptP& o, float g, float& p, float& s1, float& s2) {
  static_assert(KIND >= TFRA_OPT_SGD && KIND <= TFRA_OPT_RMSPROP, "apply_one: a kind without a rule (the last branch is FTRL's alone)");
  if (KIND == TFRA_OPT_SGD) {
    p = p - o.lr * g;
  } else if (KIND == TFRA_OPT_ADAM) {
    // m += (g-m)(1-b1); v += (g*g-v)(1-b2); p -= lr_t*m/(sqrt(v)+eps)
    s1 = s1 + (g - s1) * (1.f - o.beta1);
    s2 = s2 + (g * g - s2) * (1.f - o.beta2);
    p = p - (s1 * o.lr) / (sqrtf(s2) + o.eps);
  } else if (KIND == TFRA_OPT_ADAGRAD) {
    s1 = s1 + g * g;
    if (o.eps < 0.f) p = p - o.lr * g / sqrtf(s1);
    else p = p - o.lr * g / (sqrtf(s1) + o.eps);
  } else if (KIND == TFRA_OPT_MOMENTUM) {   // ResourceApplyMomentum: s1 = accum
    s1 = s1 * o.beta1 + g;
    p = p - s1 * o.lr;
  } else if (KIND == TFRA_OPT_NESTEROV) {   // ... with use_nesterov; beta1 * lr is rounded once, from the lr in force (d_lr)
    s1 = s1 * o.beta1 + g;
    p = p - (g * o.lr + s1 * (o.beta1 * o.lr));
  } else if (KIND == TFRA_OPT_RMSPROP) {    // ResourceApplyRMSProp: s1 = ms, s2 = mom; beta2 carries 1 - rho (tfra_mi355x.h)
    s1 = s1 + (g * g - s1) * o.beta2;
    s2 = s2 * o.beta1 + (g * o.lr) / sqrtf(s1 + o.eps);
    p = p - s2;
  } else {  // FTRL: s1 = accum, s2 = linear
    float a_new = s1 + g * g;
    float pa_new, pa;
    if (o.lr_power == -0.5f) { pa_new = sqrtf(a_new); pa = sqrtf(s1); }
    else { pa_new = powf(a_new, -o.lr_power); pa = powf(s1, -o.lr_power); }
    float sigma = (pa_new - pa) / o.lr;
    s2 = s2 + g - sigma * p;
    float q = pa_new / o.lr + 2.f * o.l2;
    p = (fabsf(s2) > o.l1) ? (sgnf(s2) * o.l1 - s2) / q : 0.f;
    s1 = a_new;
  }
}

// Rows of half / bfloat16 tables (GPU value types of the reference: hkv_hashtable_op_gpu.cu.cc:1133-1138) through the fused
// optimizers: the rule is evaluated in fp32 on the up-cast row and slots, the results are rounded to the storage type once,
// to nearest even.  ST: 0 float, 1 half, 2 bfloat16 (tfra_dtype).
template <int ST> struct Stored { typedef float T; };
template <> struct Stored<TFRA_F16> { typedef __half T; };
template <> struct Stored<TFRA_BF16> { typedef unsigned short T; };
template <int ST> __device__ __forceinline__ float load_stored(const typename Stored<ST>::T* p) { return *p; }
template <> __device__ __forceinline__ float load_stored<TFRA_F16>(const __half* p) { return __half2float(*p); }
template <> __device__ __forceinline__ float load_stored<TFRA_BF16>(const unsigned short* p) { return __uint_as_float((unsigned)*p << 16); }
template <int ST> __device__ __forceinline__ typename Stored<ST>::T to_stored(float x) { return x; }
template <> __device__ __forceinline__ __half to_stored<TFRA_F16>(float x) { return __float2half_rn(x); }
template <> __device__ __forceinline__ unsigned short to_stored<TFRA_BF16>(float x) {
  unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

// Four stored elements of a half / bfloat16 row as one 8-byte granule (element c in the low 16 bits): the same conversions as
// load_stored / to_stored, element by element.
template <int ST> __device__ __forceinline__ float bits_to_float(unsigned b);
template <> __device__ __forceinline__ float bits_to_float<TFRA_F16>(unsigned b) { return __half2float(__ushort_as_half((unsigned short)b)); }
template <> __device__ __forceinline__ float bits_to_float<TFRA_BF16>(unsigned b) { return __uint_as_float(b << 16); }
template <int ST> __device__ __forceinline__ unsigned float_to_bits(float x);
template <> __device__ __forceinline__ unsigned float_to_bits<TFRA_F16>(float x) { return __half_as_ushort(to_stored<TFRA_F16>(x)); }
template <> __device__ __forceinline__ unsigned float_to_bits<TFRA_BF16>(float x) { return to_stored<TFRA_BF16>(x); }
template <int ST> __device__ __forceinline__ float4 load_stored4(uint2 r) {
  return make_float4(bits_to_float<ST>(r.x & 0xffffu), bits_to_float<ST>(r.x >> 16), bits_to_float<ST>(r.y & 0xffffu),
                     bits_to_float<ST>(r.y >> 16));
}
template <int ST> __device__ __forceinline__ u64 to_stored4(const float4& x) {
  const unsigned lo = float_to_bits<ST>(x.x) | (float_to_bits<ST>(x.y) << 16);
  const unsigned hi = float_to_bits<ST>(x.z) | (float_to_bits<ST>(x.w) << 16);
  return ((u64)hi << 32) | lo;
}

// ---- stochastic rounding of the write-back (TFRA_OPTION_STOCHASTIC_ROUNDING): the counterpart of to_stored / to_stored4.
// The random bits are a pure function of (seed, call, key, element), formed by the splitmix64 finalizer:
//   a = mix64(seed + call * GAMMA)        once per call, on the host (Table::stoch_of) — the kernels' StochP
//   b = mix64(a ^ key)                    once per key (sr_key)
//   w = mix64(b + ((e >> 2) + 1) * GAMMA) once per granule of four elements, e = field * dim + column (sr_word)
//   r = (w >> 16 (e & 3)) & 0xffff        the element's 16 bits
// The rule: lo = x toward zero on the storage grid (continued by one step past the largest finite value, stored as infinity),
// hi the next grid value away from zero, F = 65536 (|x| - |lo|) / (|hi| - |lo|); the result is hi iff 65536 - r <= F.
// A kernel rounds this way when its trailing pack holds a StochP; without one it compiles what it always did.
constexpr u64 SR_GAMMA = 0x9E3779B97F4A7C15ull;
struct StochP { u64 a; };
__host__ __device__ __forceinline__ u64 sr_mix64(u64 z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ u64 sr_key(const StochP& sr, i64 key) { return sr_mix64(sr.a ^ (u64)key); }
__device__ __forceinline__ u64 sr_word(u64 b, unsigned e) { return sr_mix64(b + (u64)((e >> 2) + 1u) * SR_GAMMA); }
__device__ __forceinline__ unsigned sr_bits(u64 w, unsigned e) { return (unsigned)(w >> (16u * (e & 3u))) & 0xffffu; }

// the stored bits of x with the 16 random bits r
template <int ST> __device__ __forceinline__ unsigned float_to_bits_sr(float x, unsigned r);
template <> __device__ __forceinline__ unsigned float_to_bits_sr<TFRA_BF16>(float x, unsigned r) {
  const unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) >= 0x7f800000u) return to_stored<TFRA_BF16>(x);   // infinity, NaN: as nearest-even stores them
  return (u + r) >> 16;   // F = the low half of the bits: the carry is hi (0x7f7f.... + carry = infinity, the continued step)
}
template <> __device__ __forceinline__ unsigned float_to_bits_sr<TFRA_F16>(float x, unsigned r) {
  const unsigned u = __float_as_uint(x), au = u & 0x7fffffffu, sign = (u >> 16) & 0x8000u;
  if (au >= 0x47800000u) return __half_as_ushort(to_stored<TFRA_F16>(x));   // |x| >= 2^16 (the continued step), infinity, NaN
  // normal halves, 2^-14 <= |x| < 2^16: F = 8 x the low 13 bits; add r >> 3, clear them, re-bias the exponent (2^16 comes out as 0x7c00)
  const unsigned nrm = (((au + (r >> 3)) & ~0x1fffu) - 0x38000000u) >> 13;
  // subnormal halves, |x| < 2^-14: the grid is the multiples of 2^-24; |x| 2^24 = lo + fraction, both exact in fp32
  const float t = __uint_as_float(min(au, 0x38800000u)) * 16777216.f;
  const float lo = truncf(t);
  const unsigned sub = (unsigned)lo + (((float)(65536u - r) <= (t - lo) * 65536.f) ? 1u : 0u);   // (1024 = 0x0400 = 2^-14)
  return sign | (au >= 0x38800000u ? nrm : sub);
}
template <int ST> __device__ __forceinline__ typename Stored<ST>::T to_stored_sr(float x, unsigned r);
template <> __device__ __forceinline__ __half to_stored_sr<TFRA_F16>(float x, unsigned r) {
  return __ushort_as_half((unsigned short)float_to_bits_sr<TFRA_F16>(x, r));
}
template <> __device__ __forceinline__ unsigned short to_stored_sr<TFRA_BF16>(float x, unsigned r) {
  return (unsigned short)float_to_bits_sr<TFRA_BF16>(x, r);
}
// four elements of one granule: element c of the granule takes bits 16 c .. 16 c + 15 of w
template <int ST> __device__ __forceinline__ u64 to_stored4_sr(const float4& x, u64 w) {
  const unsigned wl = (unsigned)w, wh = (unsigned)(w >> 32);
  const unsigned lo = float_to_bits_sr<ST>(x.x, wl & 0xffffu) | (float_to_bits_sr<ST>(x.y, wl >> 16) << 16);
  const unsigned hi = float_to_bits_sr<ST>(x.z, wh & 0xffffu) | (float_to_bits_sr<ST>(x.w, wh >> 16) << 16);
  return ((u64)hi << 32) | lo;
}

// The rounding axis of a kernel's trailing pack: whether it holds a StochP, and that record (a pack without one: a = 0, unused)
template <class... XS> struct HasStoch { static constexpr bool v = (false || ... || std::is_same<XS, StochP>::value); };
template <class... XS>
__device__ __forceinline__ StochP stoch_in(const XS&... xs) {
  StochP sr{0};
  auto take = [&](const auto& x) { if constexpr (std::is_same<std::decay_t<decltype(x)>, StochP>::value) sr = x; };
  (take(xs), ...);
  return sr;
}

// score strategy of the table + its current epoch (update_score)
struct ScoreP { int strategy; u64 epoch; int bounded; };  // bounded: 0 / 1 / 2 (dense), see locate_or_claim_from

// Slot fields a rule owns — the ONE place: the kernels (NSlots) and the hosts' argument checks both read it
constexpr int opt_slots(int kind) {
  return kind == TFRA_OPT_SGD ? 0 : (kind == TFRA_OPT_ADAGRAD || kind == TFRA_OPT_MOMENTUM || kind == TFRA_OPT_NESTEROV) ? 1 : 2;
}
template <int KIND> struct NSlots { static constexpr int v = opt_slots(KIND); };


}  // namespace tfra
