// sampling: one token per row of logits -- temperature, an optional top-k or top-p cut, one multinomial draw from the repository's
// counter-based PRNG -- and, with a mask, the nearest-code token resampling of the reference's codec.py:121-180.
// One launch for all R rows; no workspace, nothing allocated, synchronised or read back.
//
//   * the row stays in registers: a lane keeps SP_SLOTS = 16 entries (the sortable key of the logit and the weight), a wave 1024.  Entry
//     idx of the row is slot (idx / 64) % 16 of lane idx % 64 of wave idx / 1024: a CHUNK is 64 consecutive indices, one slot of one wave,
//     and the loads of a chunk are one coalesced 256-byte request.
//   * two forms, chosen on the host from C alone (sp_form):
//       1  C <= 1024: one wave per row, four rows per 256-thread workgroup, no LDS and no barrier;
//       2  1024 < C <= 16384: one workgroup of ceil(C / 1024) waves per row; the waves exchange one word per reduction through LDS.
//     The switch is where a row stops fitting the 16 slots of one wave.  The codecs' codebooks (1024 here; 2048 and 4096 go to form 2 with
//     2 and 4 waves) come with hundreds of thousands of rows, a language model's vocabulary with few: more waves per row is what cuts its latency.
//   * weights: w = exp2((l - max) * (log2 e / temp)); -inf gives 0.  A row with a NaN or without a finite maximum returns -1.
//   * the kept set S: entries are ranked by value descending, ties by ascending index.  The key of a logit is its bit pattern made
//     monotone (sp_key; -0 is read as +0), so the ranking is decided on bits.  A 32-step search finds the largest key T whose entries
//     at or above it count at least k (top-k: the sums are of 1.0f, exact) or weigh more than p Z (top-p); S is every entry above T and
//     the first m entries equal to T by index -- m = k - (the count above T), or the ties whose mass before, above + rank * w, is <= p Z.
//     top_p >= 1 keeps everything (mass before < Z holds for every entry without any sum), as does no cut.
//   * every sum is fp32 in ONE structure (SpRow::sum): a lane adds its 16 slots in order, the 64 lanes by an xor butterfly, the waves
//     in order.  Each step is monotone in its inputs, so the masked sums of the search are monotone in the threshold.
//   * the draw: t = u Z_S.  The prefix sums are fp32: a Hillis-Steele wave scan over the 64 entries of a chunk (p), a wave scan over the
//     wave's 16 chunk totals (P), then a carry across waves added in wave order (B).  Level 1 picks the first chunk with a positive total
//     whose B + P exceeds t (none: the last chunk with a positive total); level 2 the first entry of that chunk with a positive weight
//     whose (B + P of the chunk before) + p exceeds t (none: the last entry with a positive weight).  The result therefore always
//     has a positive weight and lies in S, whatever the rounding; where it can differ from the exact statement is within the rounding of
//     these sums of the interval's ends (tests/sampling_ref.py: the draw margin).
//   * random words: word i = mix(key + (i + 1) * GOLDEN), audiocodecs_amd/prng.py's _draw; row r uses words 2 (offset + r) (mask) and
//     2 (offset + r) + 1 (draw); u = (word >> 40) * 2^-24.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ac {

constexpr int SP_MIN_C = 2;
constexpr int SP_MAX_C = 16384;
constexpr int SP_SLOTS = 16;                          // entries a lane keeps
constexpr int SP_WAVE_C = 64 * SP_SLOTS;              // entries a wave keeps: the form switch
constexpr int SP_MAX_WAVES = SP_MAX_C / SP_WAVE_C;    // 16: the largest workgroup of form 2 has 1024 threads
constexpr int SP_ROWS_PER_BLOCK = 4;                  // form 1
constexpr long long SP_MAX_ROWS = (1ll << 31) - 1;    // rows a launch takes (form 2's grid)

// C is in range
__host__ __device__ inline int sp_form(int C) { return C <= SP_WAVE_C ? 1 : 2; }
__host__ __device__ inline int sp_waves(int C) { return (C + SP_WAVE_C - 1) / SP_WAVE_C; }

struct SampleParams {
    const float* logits;
    long long row_stride;
    const long long* row_index;      // [R] or null
    long long R;
    int C;
    float scale;                     // log2(e) / temp
    int top_k;                       // 0 = off
    float top_p;                     // < 0 = off
    unsigned long long key, offset;
    const long long* offset_dev;     // [1] or null
    float mask_p;                    // < 0 = no mask
    const long long* fallback;       // [R], with a mask
    long long* out;                  // [R]
};

__device__ __forceinline__ unsigned long long sp_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// word i of the stream as a uniform in [0, 1): 24 bits, exact in fp32
__device__ __forceinline__ float sp_uniform(unsigned long long key, unsigned long long i) {
    const unsigned long long w = sp_mix(key + (i + 1ull) * 0x9E3779B97F4A7C15ull);
    return (float)(unsigned)(w >> 40) * 5.9604644775390625e-08f;
}

// the logit's bits, monotone: a < b as floats <=> sp_key(a) < sp_key(b) as unsigned (no NaN, -0 already read as +0).  Every real key is
// above 0, the key of the slots past the row's end.
__device__ __forceinline__ unsigned sp_key(float l) {
    const unsigned u = __float_as_uint(l);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float sp_wave_sum(float x) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) x += __shfl_xor(x, sh);
    return x;
}

// inclusive Hillis-Steele scan over the 64 lanes
__device__ __forceinline__ float sp_wave_scan(float x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// What the waves of a row share.  Form 2: every wave leaves one word per round in LDS and reads all of them behind ONE barrier; the rounds
// alternate between two buffers, so a wave that is already writing round n + 1 cannot overtake one still reading round n (and round n + 2
// is behind the barrier of round n + 1).  Form 1: there is one wave and nothing to share.
template <bool MULTI>
struct SpRow {
    unsigned* sh;      // [2][SP_MAX_WAVES]
    int wave, nw, lane;
    int round = 0;

    __device__ __forceinline__ const unsigned* exchange(unsigned mine) {
        unsigned* b = sh + (round & 1) * SP_MAX_WAVES;
        ++round;
        if (lane == 0) b[wave] = mine;
        __syncthreads();
        return b;
    }

    // the row's sum of one value per lane: lanes by butterfly, waves in order
    __device__ __forceinline__ float sum(float acc) {
        const float s = sp_wave_sum(acc);
        if constexpr (!MULTI) {
            return s;
        } else {
            const unsigned* b = exchange(__float_as_uint(s));
            float tot = 0.0f;
            for (int j = 0; j < nw; ++j) tot += __uint_as_float(b[j]);
            return tot;
        }
    }
};

template <bool MULTI>
__device__ __forceinline__ void sp_sample_row(const SampleParams& p, long long r, SpRow<MULTI> row) {
    const int lane = row.lane, wave = row.wave;
    const bool writer = lane == 0 && wave == 0;
    const unsigned long long e = p.offset + (p.offset_dev ? (unsigned long long)*p.offset_dev : 0ull) + (unsigned long long)r;
    if (p.mask_p >= 0.0f && !(sp_uniform(p.key, 2ull * e) < p.mask_p)) {      // (the same for every thread of the row)
        if (writer) p.out[r] = p.fallback[r];
        return;
    }
    const float* src = p.logits + (p.row_index ? p.row_index[r] : r) * p.row_stride;
    const int first = wave * SP_WAVE_C + lane;
    const int nslots = (p.C - wave * SP_WAVE_C + 63) / 64;      // the wave's chunks that hold entries (the loops below stop there)

    float w[SP_SLOTS];
    unsigned key[SP_SLOTS];
    float mx = -INFINITY;
    bool nan = false;
#pragma unroll
    for (int i = 0; i < SP_SLOTS; ++i) {
        const int idx = first + i * 64;
        float l = -INFINITY;
        key[i] = 0u;
        if (idx < p.C) {
            l = src[idx];
            nan |= l != l;
            if (l == 0.0f) l = 0.0f;      // -0 ties with +0
            key[i] = sp_key(l);
            mx = fmaxf(mx, l);
        }
        w[i] = l;
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) mx = fmaxf(mx, __shfl_xor(mx, sh));
    if (__any(nan)) mx = NAN;
    if constexpr (MULTI) {
        const unsigned* b = row.exchange(__float_as_uint(mx));
        float m = -INFINITY;
        bool bad = false;
        for (int j = 0; j < row.nw; ++j) {
            const float v = __uint_as_float(b[j]);
            bad |= v != v;
            m = fmaxf(m, v);
        }
        mx = bad ? NAN : m;
    }
    if (!(fabsf(mx) < INFINITY)) {      // a NaN in the row, +inf, or nothing above -inf
        if (writer) p.out[r] = -1;
        return;
    }
#pragma unroll
    for (int i = 0; i < SP_SLOTS; ++i) w[i] = __builtin_amdgcn_exp2f((w[i] - mx) * p.scale);      // (-inf and the slots past the end: 0)

    if (p.top_k > 0 || (p.top_p >= 0.0f && p.top_p < 1.0f)) {
        const bool by_count = p.top_k > 0;
        float bound = (float)p.top_k - 0.5f;      // count >= k  <=>  count > k - 0.5
        if (!by_count) {
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < SP_SLOTS; ++i) acc += w[i];
            bound = p.top_p * row.sum(acc);
        }
        // T: the largest key with sum(key >= T) > bound (the sum of everything is: k <= C, p < 1)
        unsigned T = 0u;
        for (unsigned bit = 0x80000000u; bit; bit >>= 1) {
            const unsigned cand = T | bit;
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < SP_SLOTS; ++i) {
                if (i < nslots) acc += key[i] >= cand ? (by_count ? 1.0f : w[i]) : 0.0f;
            }
            if (row.sum(acc) > bound) T = cand;
        }
        float acc = 0.0f;
        unsigned ties = 0;
#pragma unroll
        for (int i = 0; i < SP_SLOTS; ++i) {
            acc += key[i] > T ? (by_count ? 1.0f : w[i]) : 0.0f;
            ties += (unsigned)__popcll(__ballot(key[i] == T));
        }
        const float above = row.sum(acc);      // what is ranked before every entry equal to T (<= bound)
        unsigned rank0 = 0;                    // the ties at lower indices than this wave's
        if constexpr (MULTI) {
            const unsigned* b = row.exchange(ties);
            for (int j = 0; j < wave; ++j) rank0 += b[j];
        }
        const unsigned keep = (unsigned)p.top_k - (unsigned)above;      // (top-k: the ties that stay)
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (int i = 0; i < SP_SLOTS; ++i) {
            const unsigned long long tie = __ballot(key[i] == T);
            const unsigned rank = rank0 + (unsigned)__popcll(tie & below);
            rank0 += (unsigned)__popcll(tie);
            const bool kept = by_count ? rank < keep : above + (float)rank * w[i] <= bound;
            if (!(key[i] > T || (key[i] == T && kept))) w[i] = 0.0f;
        }
    }

    // chunk totals (lane i keeps chunk i's), their prefix in the wave, the carry across waves
    float total = 0.0f;
#pragma unroll
    for (int i = 0; i < SP_SLOTS; ++i) {
        if (i < nslots) {
            const float t63 = __shfl(sp_wave_scan(w[i], lane), 63);
            if (lane == i) total = t63;
        }
    }
    const float P = sp_wave_scan(total, lane);      // (lanes >= 16 add zeros: lane 63 holds the wave's total)
    const float wave_total = __shfl(P, 63);
    float B = 0.0f, Z = wave_total;
    if constexpr (MULTI) {
        const unsigned* b = row.exchange(__float_as_uint(wave_total));
        Z = 0.0f;
        for (int j = 0; j < row.nw; ++j) {
            if (j == wave) B = Z;
            Z += __uint_as_float(b[j]);
        }
    }
    const float t = sp_uniform(p.key, 2ull * e + 1ull) * Z;

    // level 1: the chunk
    const bool live = lane < SP_SLOTS && total > 0.0f;
    const unsigned long long hit = __ballot(live && B + P > t), any = __ballot(live);
    int chunk_hit = hit ? wave * SP_SLOTS + (__ffsll((long long)hit) - 1) : 0xFFFF;
    int chunk_last = any ? wave * SP_SLOTS + (63 - __clzll((long long)any)) : -1;
    if constexpr (MULTI) {
        const unsigned* b = row.exchange((unsigned)chunk_hit << 16 | (unsigned)(chunk_last + 1));
        chunk_hit = 0xFFFF;
        chunk_last = -1;
        for (int j = 0; j < row.nw; ++j) {
            const int h = (int)(b[j] >> 16), l = (int)(b[j] & 0xFFFFu) - 1;
            chunk_hit = h < chunk_hit ? h : chunk_hit;
            chunk_last = l > chunk_last ? l : chunk_last;
        }
    }
    const int chunk = chunk_hit != 0xFFFF ? chunk_hit : chunk_last;      // (the maximum has weight 1 and is in S: some chunk is live)
    if (chunk < 0 || chunk / SP_SLOTS != wave) return;

    // level 2: the entry, in the wave that keeps the chunk
    const int slot = chunk % SP_SLOTS;
    float x = 0.0f;
#pragma unroll
    for (int i = 0; i < SP_SLOTS; ++i) x = i == slot ? w[i] : x;
    const float pfx = sp_wave_scan(x, lane);
    const float before = __shfl(P, slot > 0 ? slot - 1 : 0);
    const float base = B + (slot > 0 ? before : 0.0f);
    const unsigned long long pos = __ballot(x > 0.0f), over = __ballot(x > 0.0f && base + pfx > t);
    const int pick = over ? __ffsll((long long)over) - 1 : 63 - __clzll((long long)pos);
    if (lane == 0) p.out[r] = (long long)chunk * 64 + pick;
}

__global__ __launch_bounds__(64 * SP_ROWS_PER_BLOCK) void sample_wave_kernel(const SampleParams p) {
    const long long r = (long long)blockIdx.x * SP_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= p.R) return;
    sp_sample_row<false>(p, r, SpRow<false>{nullptr, 0, 1, (int)(threadIdx.x & 63)});
}

// blockDim.x = 64 * sp_waves(C)
__global__ __launch_bounds__(64 * SP_MAX_WAVES) void sample_block_kernel(const SampleParams p) {
    __shared__ unsigned sh[2 * SP_MAX_WAVES];
    sp_sample_row<true>(p, (long long)blockIdx.x, SpRow<true>{sh, (int)(threadIdx.x >> 6), (int)(blockDim.x >> 6), (int)(threadIdx.x & 63)});
}

}  // namespace ac
