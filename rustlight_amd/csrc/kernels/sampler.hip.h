// sampler.hip.h — the samplers the draw sites of the stage functions (stages.hip.h) and of `ao` / `direct` (mc.hip.h) are written against:
//   smp_next(r)   = Sampler::next()    one f32 in [0, 1)
//   smp_next2d(r) = Sampler::next2d()  two of them, x then y
// Independent (samplers/independent.rs): the sample's own Rng, exactly as before — the draw sites compile to the very same code.
// Stratified  (samplers/stratified.rs, RL_STREAM_STRATIFIED): StratSampler below.
// Part of common.hip.h (after devmath / pathstate).
#pragma once

namespace rl {

// ---- independent: the sample's Rng
RL_DEV float smp_next(Rng& r) { return rng_next_f32(r); }
RL_DEV V2 smp_next2d(Rng& r) { V2 v; v.x = rng_next_f32(r); v.y = rng_next_f32(r); return v; }
RL_DEV unsigned smp_flag_bits(const Rng&) { return 0u; }

// ---- stratified (StratifiedSampler::create(spp, 4)): n = the power of four >= spp; 4 one-dimensional and 4 two-dimensional dimensions per
// camera sample.  Sample s of a pixel takes, in 1D dimension k, stratum (pi_k(s) + r_k) mod n and in 2D dimension k cell (sigma_k(s) + r'_k) mod n
// = (cell / sqrt n, cell % sqrt n), jittered by draws of the sample's own Rng; pi_k / sigma_k are keyed bijections of [0, n) (Kensler's permute) and
// r_k a keyed rotation, both derived from a hash of the pixel's seed (item_seed), so every sample's stratum is uniform over the key and every value
// is U[0, 1) marginally.  The k-th next() of a sample reads 1D dimension k, the k-th next2d() 2D dimension k (independent counters); past the fourth
// dimension of a kind the plain Rng draws.  The reference shuffles arrays it fills from `random()`; this sampler is a pure function of
// (block seeds, pixel, sample index, spp, seed_variant): what pipeline, split, sharding or device renders a sample does not change a bit.
// Its only state besides the Rng is the two counters: ST_SMP_SHIFT bits of U_FLAGS between stage launches.
static constexpr unsigned kStratDims = 4u;
enum : unsigned { ST_SMP_SHIFT = 16u };    // U_FLAGS bits 16-18: 1D dimensions used, 19-21: 2D dimensions used (stratified kernels only)

struct StratSampler {
    Rng rng;                     // the sample's own sampler (forked as in RL_STREAM_PER_SAMPLE): the jitter, and every draw past the strata
    unsigned long long key;      // per pixel: strat_pixel_key(item_seed)
    unsigned s;                  // sample index
    unsigned lg;                 // log2 n (even)
    unsigned used1, used2;       // dimensions of each kind taken so far by this sample
};

RL_DEV unsigned long long strat_mix64(unsigned long long z) {      // SplitMix64's finaliser
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
RL_DEV unsigned long long strat_pixel_key(unsigned long long item_seed) { return strat_mix64(item_seed ^ 0x5851f42d4c957f2dull); }
// log2 of the power of four >= spp (spp <= 2^30: rl_render_* refuse more in this mode)
RL_DEV unsigned strat_log2n(unsigned spp) {
    const unsigned l2 = spp <= 1u ? 0u : 32u - (unsigned)__clz(spp - 1u);    // ceil(log2 spp)
    return (l2 + 1u) & ~1u;
}
// Kensler, "Correlated Multi-Jittered Sampling" (2013), permute(): a keyed bijection of [0, w] for w = 2^k - 1 — every step maps the low k bits
// to themselves bijectively, so no cycle-walking is needed
RL_DEV unsigned strat_permute(unsigned i, unsigned w, unsigned p) {
    i ^= p; i *= 0xe170893du; i ^= p >> 16; i ^= (i & w) >> 4;
    i ^= p >> 8; i *= 0x0929eb3fu; i ^= p >> 23; i ^= (i & w) >> 1;
    i *= 1u | p >> 27; i *= 0x6935fa69u; i ^= (i & w) >> 11; i *= 0x74dcb303u;
    i ^= (i & w) >> 2; i *= 0x9e501cc3u; i ^= (i & w) >> 2; i *= 0xc860a3dfu;
    i &= w; i ^= i >> 5;
    return i & w;
}
// stratum of sample s in dimension `dim` (0-3: 1D, 4-7: 2D)
RL_DEV unsigned strat_stratum(const StratSampler& t, unsigned dim) {
    const unsigned long long h = strat_mix64(t.key + (unsigned long long)(dim + 1u) * 0x9e3779b97f4a7c15ull);
    const unsigned w = t.lg ? 0xffffffffu >> (32u - t.lg) : 0u;
    return (strat_permute(t.s & w, w, (unsigned)h) + (unsigned)(h >> 32)) & w;
}
// (stratum + U) / 2^lg with U = the 24-bit draw of Sampler::next(); the sum is truncated to f32's 24 bits instead of rounded (a round-up would land
// on the next stratum), then clamped to 1 - f32::EPSILON as stratified.rs does
RL_DEV float strat_value(unsigned stratum, Rng& rng, unsigned lg) {
    unsigned long long x = ((unsigned long long)stratum << 24) | (rng_next_u64(rng) >> 40);
    const int bits = 64 - __clzll((long long)(x | 1ull));
    if (bits > 24) { const int sh = bits - 24; x = (x >> sh) << sh; }
    const float scale = __uint_as_float((127u - 24u - lg) << 23);          // 2^-(24 + lg), exact
    return fminf((float)x * scale, 1.0f - 1.0f / 8388608.0f);
}
RL_DEV float smp_next(StratSampler& t) {
    if (t.used1 >= kStratDims) return rng_next_f32(t.rng);
    const unsigned st = strat_stratum(t, t.used1++);
    return strat_value(st, t.rng, t.lg);
}
RL_DEV V2 smp_next2d(StratSampler& t) {
    V2 v;
    if (t.used2 >= kStratDims) { v.x = rng_next_f32(t.rng); v.y = rng_next_f32(t.rng); return v; }
    const unsigned cell = strat_stratum(t, kStratDims + t.used2++), h = t.lg >> 1;
    v.x = strat_value(cell >> h, t.rng, h);                    // chunks_mut order: cell c -> (c / sqrt n, c % sqrt n)
    v.y = strat_value(cell & ((1u << h) - 1u), t.rng, h);
    return v;
}
RL_DEV unsigned smp_flag_bits(const StratSampler& t) { return (t.used1 | (t.used2 << 3)) << ST_SMP_SHIFT; }
RL_DEV StratSampler strat_begin(const RenderConst& rc, const Rng& rng, unsigned pixel_item, unsigned s) {
    StratSampler t;
    t.rng = rng; t.key = strat_pixel_key(rc.item_seed[pixel_item]); t.s = s; t.lg = strat_log2n(rc.spp); t.used1 = 0u; t.used2 = 0u;
    return t;
}

// How the stage functions take a sampler from the path state and give it back (SMP = Rng: the Q_R0 state, nothing else).
template <class SMP> struct SmpState;
template <> struct SmpState<Rng> {
    RL_DEV static Rng begin(const RenderConst&, const Rng& rng, unsigned, unsigned) { return rng; }
    template <class PS> RL_DEV static Rng load(const RenderConst&, PS& ps, unsigned) { return load_rng(ps, Q_R0); }
};
template <> struct SmpState<StratSampler> {
    RL_DEV static StratSampler begin(const RenderConst& rc, const Rng& rng, unsigned pixel_item, unsigned s) { return strat_begin(rc, rng, pixel_item, s); }
    template <class PS> RL_DEV static StratSampler load(const RenderConst& rc, PS& ps, unsigned flags) {
        const unsigned item = PU(U_ITEM);
        StratSampler t = strat_begin(rc, load_rng(ps, Q_R0), rc.split > 1u ? item / rc.split : item, PU(U_SAMPLE));
        t.used1 = (flags >> ST_SMP_SHIFT) & 7u; t.used2 = (flags >> (ST_SMP_SHIFT + 3u)) & 7u;
        return t;
    }
};
template <class PS> RL_DEV void smp_store(PS& ps, const Rng& r) { store_rng(ps, Q_R0, r); }
template <class PS> RL_DEV void smp_store(PS& ps, const StratSampler& t) { store_rng(ps, Q_R0, t.rng); }

}  // namespace rl
