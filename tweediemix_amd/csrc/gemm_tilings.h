// gemm_tilings.h -- the tilings of the bf16 / fp8 GEMM and the 3x3 convolution (tmix.h TMIX_TILE_*): ONE row per id, and the resolver that turns a
// requested id plus the traits of a launch into the kernel that runs (gemm_conv.hip).  Host only: no device code, no HIP types.
// A new tiling is a new row here, its instantiation in the row's group, and its enum value in include/tmix.h.
#pragma once

namespace tmix_gemm {

constexpr int NUM_CFG = 26;

enum Loop : unsigned char {
    LOCKSTEP,        // all waves stage a K-tile, wait, multiply it (gemm_conv_kernel, PH = 0; on e4m3 operands PH = 4 / 5)
    PHASE_OFFSET,    // eight waves, K slices of 32 through a four-slot ring, the second wave of every SIMD one barrier behind the first (PH = 1; e4m3: 2 / 3)
    OWN_KERNEL       // not an instantiation of gemm_conv_kernel: an eligibility predicate next to the kernel says which launches it runs
};
enum : unsigned char { NO_GROUP = 255 };      // Tiling::group of the retired ids and of the tilings with a kernel of their own
// what a tiling is compiled for; a launch that needs a capability its tiling lacks runs as the row's fallback
enum Cap : unsigned {
    CAP_CONV        = 1,     // has a convolution form (CONV = 1 instantiations)
    CAP_F8C         = 2,     // carries the e4m3 copy of C (TMIX_F8_COPY_OUT): compiled into the tilings with registers to spare for it
    CAP_NARROW_T    = 4,     // narrow (unstaged) stores of the transposed region: square wave tiles only
    CAP_CS          = 8,     // has the instantiations that leave column statistics (cs_out)
    CAP_F8_LOCKSTEP = 16,    // has a lock-step form on e4m3 operands (gemm_inst_5.hip): rows of 128 K values
    CAP_SC          = 32     // its convolution form carries shortcut taps
};

struct Tiling {
    short bm, bn;                 // workgroup tile
    Loop loop;
    unsigned char group;          // the translation unit gemm_inst_<group>.hip that instantiates it
    unsigned char lw;             // loader waves next to the math waves (live ids)
    unsigned char runs_as;        // the id itself, or what a retired / reserved id runs as
    unsigned caps;
    unsigned char fb, fb_conv;    // fallback of a GEMM / a convolution that needs a capability this tiling lacks (own kernels: that they cannot run); 0 = none needed
};

constexpr unsigned CAPS_PLAIN = CAP_CONV | CAP_SC | CAP_F8C | CAP_CS;      // the lock-step tilings without loader waves: every epilogue family, GEMM and convolution

constexpr Tiling TILINGS[NUM_CFG + 1] = {
    //  bm   bn  loop          group     lw runs_as caps                                   fb  fb_conv
    {    0,   0, LOCKSTEP,     NO_GROUP, 0,  0, 0,                                        0,  0},   //  0 = AUTO: 256x128 when it still yields >= 3/4 of a CU wave, else 128x128 (the plan builder overrides per shape after timing the candidates)
    {  128, 128, LOCKSTEP,     0,        0,  1, CAPS_PLAIN | CAP_NARROW_T,                     0,  0},   //  1 = 128x128 (4 waves, 2 stages, 2 WG/CU)
    {  256, 128, LOCKSTEP,     0,        0,  2, CAPS_PLAIN | CAP_NARROW_T,                     0,  0},   //  2 = 256x128 (8 waves, 3 stages)
    {  128, 128, LOCKSTEP,     0,        0,  3, CAPS_PLAIN | CAP_NARROW_T,                     0,  0},   //  3 = 128x128 (4 waves, 4 stages, 1 WG/CU)
    {  256, 256, LOCKSTEP,     1,        0,  4, CAPS_PLAIN,                                    0,  0},   //  4 = 256x256 (8 waves, 2 stages)
    // 5 = 256x128 (4 waves of 128x64, 3 stages, 1 WG/CU), 6 = 256x256 (4 waves of 128x128, 2 stages, 1 WG/CU): one wave per SIMD with a large register tile -- on this
    // chip instructions of co-resident waves do not overlap on a SIMD, so MFMA utilisation is set by MFMAs per non-MFMA instruction, i.e. by the wave tile.
    // 6 is retired: it spilled and lost everywhere; it runs as the same tile shape over eight waves
    {  256, 128, LOCKSTEP,     1,        0,  5, CAPS_PLAIN,                                    0,  0},
    {  256, 256, LOCKSTEP,     NO_GROUP, 0,  4, 0,                                        0,  0},
    // 7 = 128x160 (4 waves of 32x160, 2 stages): N = 1280 / 640 split into 160-wide tiles gives exactly 256 / 512 tiles for this path's M = 4096 / 16384 GEMMs,
    // i.e. whole rounds on 256 CUs instead of 1.25 / 2.5
    {  128, 160, LOCKSTEP,     2,        0,  7, CAPS_PLAIN,                                    0,  0},
    // 8..11 = tilings 7, 2, 1, 4 with one extra LOADER wave (wave specialisation, see gemm_conv_kernel), retired: at 3 waves / SIMD register budget they spilled
    // (the 4-wave tilings with 128-wide wave tiles, 5 and 6, have no registers for a fifth wave on one of the SIMDs)
    {  128, 160, LOCKSTEP,     NO_GROUP, 0, 19, 0,                                        0,  0},
    {  256, 128, LOCKSTEP,     NO_GROUP, 0,  2, 0,                                        0,  0},
    {  128, 128, LOCKSTEP,     NO_GROUP, 0,  1, 0,                                        0,  0},
    {  256, 256, LOCKSTEP,     NO_GROUP, 0,  4, 0,                                        0,  0},
    // 12 = tiling 7 (128x160) with a 4-deep ring (one workgroup per CU, three K-tiles in flight: the in-sequence loop is bound by memory latency x bytes in flight,
    // and 160-wide tiles divide N = 1280 / 640 exactly)
    {  128, 160, LOCKSTEP,     2,        0, 12, CAPS_PLAIN | CAP_F8_LOCKSTEP,                  0,  0},
    // 13 = 64x160 over FIVE waves (each 64x32), 4-deep ring: 2048 x 1280 -- the half-batch launches of the 32x32 level -- is exactly 256 tiles, one per CU, where
    // 128x128 leaves 96 CUs idle (160 tiles) and 128x160 half of them
    {   64, 160, LOCKSTEP,     2,        0, 13, CAPS_PLAIN,                                    0,  0},
    // 14 = 256x320 over eight waves (wave tile 64x160): the GEGLU up-projection 2048 x 10240 is exactly 256 tiles, where 256x256 runs 320 (a quarter-full second
    // round); 128x320 over four waves was tried and lost to 128x160 everywhere.  No registers to spare for the e4m3 copy
    {  256, 320, LOCKSTEP,     3,        0, 14, CAP_CONV | CAP_SC | CAP_CS,              12,  0},
    // 15 = 32x160 over five waves (each 32x32): 1024 x 1280 -- one batch row per chain, the CFG-pair calls -- is 256 tiles (a 5-deep ring for 13 measured the same
    // as the 4-deep one)
    {   32, 160, LOCKSTEP,     3,        0, 15, CAPS_PLAIN,                                    0,  0},
    // 16 = 256x256, 17 = 256x128 with the PHASE-OFFSET mainloop: GEMM only (the im2col gather's per-row offset tables do not fit the register budget, and the conv
    // mainloop already runs at 0.8-1.0 PFLOP/s), no transposed region; bf16 and e4m3 operands.  Fallback: the nearest plain tiling
    {  256, 256, PHASE_OFFSET, 4,        0, 16, CAP_F8C,                                  4,  4},
    {  256, 128, PHASE_OFFSET, 4,        0, 17, CAP_F8C,                                  2,  2},
    // 18 = tiling 12 (128x160, 4-deep ring) with in-workgroup split-K over two wave groups (KS = 2): eight waves stage, GEMM only
    {  128, 160, LOCKSTEP,     2,        0, 18, CAP_F8C | CAP_CS,                         0, 12},
    // 19 / 20 / 21 = tiling 12 (128x160; 19: 3-deep ring) with one / two / FOUR LOADER waves next to the four math waves; with four every SIMD hosts one math wave
    // and one loader, and a K-tile's 36 LDS-DMA instructions are nine per loader.  GEMM only, except 20: it also exists for the convolution since the kernels are
    // instantiated per epilogue family (244 VGPRs, no scratch).  On e4m3 operands they carry the e4m3 copy themselves, in its straight-line form
    {  128, 160, LOCKSTEP,     3,        1, 19, CAP_CS | CAP_F8_LOCKSTEP,                12, 12},
    {  128, 160, LOCKSTEP,     3,        2, 20, CAP_CONV | CAP_SC | CAP_CS | CAP_F8_LOCKSTEP, 12, 0},
    {  128, 160, LOCKSTEP,     3,        4, 21, CAP_CS | CAP_F8_LOCKSTEP,                12, 12},
    // 22 = 256x320 with the PHASE-OFFSET mainloop (eight waves of 64x160; bf16 GEMM only, staged GEGLU / plain epilogues only: the transposed and narrow forms spill at
    // its register count): the lock-step 256x320 loop (14) stops all eight waves at every K-tile hand-over -- 79 % of the MFMA rate with the LDS-DMA ablated -- where
    // this one keeps one wave of every SIMD in its MFMA segment
    {  256, 320, PHASE_OFFSET, 4,        0, 22, 0,                                       14, 14},
    // 23 = 128x160 over 2 x 2 math waves of 64x80 on v_mfma_f32_16x16x32_bf16 + four loader waves (its own kernel: gemm_w22.hip): the staged plain bf16 epilogue only
    {  128, 160, OWN_KERNEL,   NO_GROUP, 4, 23, 0,                                       21, 12},
    // 24 / 25 = reserved: they were 256x320 on persistent workgroups and tiling 23 with an L2 prefetcher wave, both measured slower in the step (DESIGN.md 5b
    // items 5, 6) and removed; the ids stay valid and run as the tilings they were variants of (same bits)
    {  256, 320, OWN_KERNEL,   NO_GROUP, 0, 14, 0,                                       14, 14},
    {  128, 160, OWN_KERNEL,   NO_GROUP, 3, 23, 0,                                       21, 12},
    // 26 = 3x3 stride-1 convolution with the input halo patch resident in LDS (4 x 32 pixel tiles, channel-chunk-major K loop; its own kernel: gemm_convh.hip);
    // anything it does not carry runs as the loader-wave tilings 20 (conv) / 21 (GEMM)
    {  128, 160, OWN_KERNEL,   NO_GROUP, 0, 26, CAP_CONV | CAP_SC | CAP_CS,              21, 20},
};

constexpr bool tile_has(int cfg, unsigned cap) { return (TILINGS[cfg].caps & cap) != 0; }

// what the resolver relies on, so that a new row cannot break it: runs_as reaches a live id in one step; fallbacks point down the table and end on a row
// with the capability they stand in for (f8copy_tile walks fb until CAP_F8C); the columns that say one thing twice agree
constexpr bool tilings_consistent() {
    for (int i = 1; i <= NUM_CFG; ++i) {
        const Tiling& t = TILINGS[i];
        if (t.runs_as < 1 || t.runs_as > NUM_CFG || TILINGS[t.runs_as].runs_as != t.runs_as) return false;
        if (t.fb >= i || t.fb_conv >= i || tile_has(i, CAP_SC) != tile_has(i, CAP_CONV)) return false;      // (shortcut taps ride in every convolution form)
        if (t.runs_as != i) continue;
        int f = i;
        while (f && !tile_has(f, CAP_F8C)) f = TILINGS[f].fb;
        if (!f) return false;
        if (t.loop == OWN_KERNEL) {
            if (!t.fb || !t.fb_conv || TILINGS[t.fb].loop == OWN_KERNEL || !tile_has(t.fb_conv, CAP_CONV)) return false;
            continue;
        }
        if (t.group > 4 || tile_has(i, CAP_CS) != (t.loop == LOCKSTEP)) return false;                          // column statistics: the lock-step instantiations only
        if (!tile_has(i, CAP_CONV) && !tile_has(t.fb_conv, CAP_CONV)) return false;
        if (!tile_has(i, CAP_CS) && !tile_has(t.fb, CAP_CS)) return false;
    }
    return true;
}
static_assert(tilings_consistent(), "gemm_tilings.h: TILINGS");

// what the resolver needs to know of a launch (filled from the validated kernel parameters in gemm_conv.hip)
struct TileTraits {
    bool conv;
    int fp8;                                 // operands: 0 = bf16, 1 = e4m3 with one scale per A row, 2 = e4m3 with MX block scales on A
    int n_trans_begin, wide, epilogue;       // as in Params
    bool f8copy, f8out, stats_out, cs_out, rowgroup_bias;
    int M, N, K, batch;
    bool w22_ok, convh_ok;                   // w22_eligible / convh_eligible of this launch (the predicates live next to their kernels)
};
// f8: mode of the kernel's loop on e4m3 operands -- 0 = bf16, 1 / 2 = phase-offset loop with per-row / MX block scales on A, 3 / 4 = the same in the lock-step loop
struct TileChoice { int cfg, f8, err; };

// the kernel a launch with these traits runs when it asks for tile_cfg: pure (sets the thread's error string when it refuses; err = TMIX_OK otherwise)
TileChoice resolve_tile(const TileTraits& t, int tile_cfg);
// may a GEMM on e4m3 operands ask for tile_cfg and get a lock-step loop?
bool f8_lockstep(int tile_cfg, int K, bool f8out);
// the tiling that runs tile_cfg (1..NUM_CFG) for a GEMM that also leaves the e4m3 copy of C
int f8copy_tile(int tile_cfg);

}  // namespace tmix_gemm
