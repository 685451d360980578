// plan.hip -- validate() and build_plan(): from fmcw_config to the launch plan (plan.hpp).
// Host code only: no HIP call, no device state.
#include "plan.hpp"

#include <cmath>

#include "internal.hpp"

namespace fmcw {
namespace {

// K2's FAST instantiation (doppler_kernel.hpp): MTI off, |X| magnitude, no dB map, fp32 windows, and the
// 1-D CFAR (if any) at the reference geometry in fp32
bool k2_fast(const fmcw_config& c) {
  const bool cfar_ok = c.cfar_kind != FMCW_CFAR_OS1D ||
                       (c.cfar1d_ref == 8 && c.cfar1d_guard == 2 && (int)(2 * c.cfar1d_ref) - (int)c.cfar1d_rank <= 4 &&
                        !(c.compat_rtl & FMCW_COMPAT_CFAR));
  return c.mti_mode == FMCW_MTI_OFF && c.mag_mode != FMCW_MAG_AMBM && c.map_kind != FMCW_MAP_DB &&
         c.window != FMCW_WIN_Q15_RTL && cfar_ok;
}

// 2-D CFAR derived parameters
Cfar2DArgs cfar2_args(const fmcw_config& c) {
  Cfar2DArgs a{};
  a.gr = (int)c.cfar2d_guard_range;
  a.gd = (int)c.cfar2d_guard_doppler;
  a.hr = (int)(c.cfar2d_ref_range + c.cfar2d_guard_range);
  a.hd = (int)(c.cfar2d_ref_doppler + c.cfar2d_guard_doppler);
  a.n_ref = (2 * a.hr + 1) * (2 * a.hd + 1) - (2 * a.gr + 1) * (2 * a.gd + 1);
  // rank_idx = N_REF * RANK_PCT / 100, clamped to N_REF - 1 (os_cfar_2d.vhd:181-182); 64-bit
  a.rank = (int)std::min<int64_t>((int64_t)a.n_ref * c.cfar2d_rank_pct / 100, (int64_t)a.n_ref - 1);
  a.sc_min = (float)c.cfar2d_scale_min;
  a.sc_nom = (float)c.cfar2d_scale_nom;
  a.sc_max = (float)c.cfar2d_scale_max;
  a.override_ = (int)c.cfar2d_scale_override;
  a.compat = (c.compat_rtl & FMCW_COMPAT_CFAR) != 0;
  a.s_min = a.override_ ? (float)a.override_ : std::min(a.sc_min, std::min(a.sc_nom, a.sc_max));
  return a;
}

Cfar2Info pick_cfar2(const fmcw_config& c, const Cfar2DArgs& a) {
  return cfar2_info(c.n_doppler, a.hd, a.gd, a.hr, a.gr, a.compat != 0);
}

Cfar1DArgs cfar1_args(const fmcw_config& c) {
  Cfar1DArgs a{};
  a.enabled = c.cfar_kind == FMCW_CFAR_OS1D;
  a.ref = (int)c.cfar1d_ref;
  a.guard = (int)c.cfar1d_guard;
  a.rank = (int)c.cfar1d_rank;
  a.alpha = c.cfar1d_alpha;
  a.compat = (c.compat_rtl & FMCW_COMPAT_CFAR) != 0;
  return a;
}

const char* range_kind_name(int kind) {
  return kind == kRangePx ? "k_range_px" : kind == kRangeSeq ? "k_range_sq" : "k_range";
}

// Frames per K1 -> K2 chunk.  With chunk_frames 0 (auto): the corner-turned spectrum of a chunk
// is written by K1 and read back by K2 right after; kept to ~13/16 of the 256 MiB Infinity Cache
// (MALL), K2's reads hit there.  Measured on config 2 (round 2, 1024 frames per step): K2 0.63
// us/frame at 128 frames (256 MiB), 0.57 at 96, 0.55 at 108-120, 0.81 from 256 frames up (reads
// from HBM).  Round 4, same box, 3 runs each (profiles/r04/chunk/): 96 frames 807.7-809.6 k
// frames/s, 104 frames 814.8-820.0 k, 112 frames 810.3-819.5 k -- so 208 MiB, without round 2's
// rounding down to whole rounds of K2's grid (96 frames), which no longer paid.  Configs 3 / 5
// (64 MiB per frame) keep 3 frames.
uint32_t chunk_frames(const fmcw_config& c, size_t frame_inter) {
  constexpr size_t kMallBudget = 208u << 20;
  const size_t ch = c.chunk_frames ? c.chunk_frames : std::max<size_t>(1, kMallBudget / frame_inter);
  // K1 / K2 address a launch's spectrum with 32-bit byte offsets (buffer loads and stores)
  const size_t cap32 = ((size_t)1 << 32) / frame_inter - 1;
  return (uint32_t)std::max<size_t>(1, std::min({ch, (size_t)c.max_frames, cap32}));
}

}  // namespace

int validate(const fmcw_config& c) {
  if (int rc = check_map_dims(c.n_range, c.n_doppler)) return rc;
  if (c.n_rx < 1 || c.n_rx > 64) return fail(FMCW_EINVAL, "n_rx=%u: must be in [1, 64]", c.n_rx);
  if (c.in_dtype < FMCW_IN_F32 || c.in_dtype > FMCW_IN_I16)
    return fail(FMCW_EINVAL, "in_dtype=%d unknown", c.in_dtype);
  if (c.window != FMCW_WIN_NONE && c.window != FMCW_WIN_HAMMING && c.window != FMCW_WIN_Q15_RTL)
    return fail(FMCW_EINVAL, "window=%d unknown", c.window);
  if (c.window == FMCW_WIN_Q15_RTL && c.in_dtype != FMCW_IN_I16)
    return fail(FMCW_EINVAL, "window Q15_RTL windows int16 ADC words: needs in_dtype I16");
  if (c.mag_mode != FMCW_MAG_ABS && c.mag_mode != FMCW_MAG_AMBM)
    return fail(FMCW_EINVAL, "mag_mode=%d unknown", c.mag_mode);
  if (c.mag_mode == FMCW_MAG_AMBM && c.n_rx != 1)
    return fail(FMCW_EINVAL, "mag_mode AMBM is defined for n_rx == 1 only");
  if (c.map_kind != FMCW_MAP_LINEAR && c.map_kind != FMCW_MAP_DB)
    return fail(FMCW_EINVAL, "map_kind=%d unknown", c.map_kind);
  if (c.mti_mode != FMCW_MTI_OFF && c.mti_mode != FMCW_MTI_2PULSE && c.mti_mode != FMCW_MTI_3PULSE)
    return fail(FMCW_EINVAL, "mti_mode=%d unknown (0 off, 2 or 3 pulse)", c.mti_mode);
  if (range_info(c.n_range, c.in_dtype, c.window, FMCW_SPEC_F32, kRangePx).T > (int)c.n_doppler)
    return fail(FMCW_EINVAL, "n_doppler=%u smaller than the range kernel's chirp group", c.n_doppler);
  if (c.max_frames < 1) return fail(FMCW_EINVAL, "max_frames must be >= 1");
  if (c.cfar_kind == FMCW_CFAR_OS1D) {
    if (c.cfar1d_ref < 1 || c.cfar1d_rank >= 2 * c.cfar1d_ref)
      return fail(FMCW_EINVAL, "1-D CFAR: need ref >= 1 and rank < 2*ref");
    if (2 * (c.cfar1d_ref + c.cfar1d_guard) + 1 > c.n_doppler)
      return fail(FMCW_EINVAL, "1-D CFAR window wider than n_doppler");
    if (!(c.cfar1d_alpha > 0.f)) return fail(FMCW_EINVAL, "1-D CFAR alpha must be > 0");
    if ((c.compat_rtl & FMCW_COMPAT_CFAR) &&
        !(c.cfar1d_alpha == std::floor(c.cfar1d_alpha) && c.cfar1d_alpha <= 16384.f))
      return fail(FMCW_EINVAL, "compat CFAR: alpha is the integer SCALING_MULT (1..16384)");
  } else if (c.cfar_kind == FMCW_CFAR_OS2D) {
    if (c.cfar2d_rank_pct > 100) return fail(FMCW_EINVAL, "2-D CFAR: rank_pct %u > 100", c.cfar2d_rank_pct);
    if (c.cfar2d_ref_range > 64 || c.cfar2d_ref_doppler > 64 || c.cfar2d_guard_range > 64 ||
        c.cfar2d_guard_doppler > 64)
      return fail(FMCW_EINVAL, "2-D CFAR window extents out of range");
    const Cfar2DArgs a = cfar2_args(c);
    if (a.n_ref < 1 || a.n_ref > 128)
      return fail(FMCW_EINVAL, "2-D CFAR: %d reference cells (supported 1..128)", a.n_ref);
    if (2 * a.hd + 1 > (int)c.n_doppler)
      return fail(FMCW_EINVAL, "2-D CFAR window wider than n_doppler");
    if (c.cfar2d_scale_override > 7)
      return fail(FMCW_EINVAL, "scale_override is a 3-bit port (0..7)");
    if (pick_cfar2(c, a).smem > 160 * 1024)
      return fail(FMCW_EINVAL, "2-D CFAR range extent too large for LDS");
  } else if (c.cfar_kind != FMCW_CFAR_NONE) {
    return fail(FMCW_EINVAL, "cfar_kind=%d unknown", c.cfar_kind);
  }
  if (c.compat_rtl & ~(uint32_t)(FMCW_COMPAT_CFAR | FMCW_COMPAT_MTI))
    return fail(FMCW_EINVAL, "compat_rtl=0x%x: unknown bits", c.compat_rtl);
  if ((c.compat_rtl & FMCW_COMPAT_MTI) && c.mti_mode == FMCW_MTI_OFF)
    return fail(FMCW_EINVAL, "compat MTI needs mti_mode 2 or 3");
  if (c.range_shift > 13) return fail(FMCW_EINVAL, "range_shift=%u: must be in [0, 13]", c.range_shift);
  if (c.spectrum_dtype != FMCW_SPEC_F32 && c.spectrum_dtype != FMCW_SPEC_F16 && c.spectrum_dtype != FMCW_SPEC_S48)
    return fail(FMCW_EINVAL, "spectrum_dtype=%d unknown", c.spectrum_dtype);
  if (c.spectrum_dtype == FMCW_SPEC_S48) {
    // one exponent per chirp group of a range bin (a quad of a K1 tile row at n_range <= 1024, a
    // pair above): the group must be one K2 lane group (n_doppler >= 64), and no MTI (the
    // canceller reads neighbouring chirps from other lanes of the group)
    if (c.n_doppler < 64) return fail(FMCW_EINVAL, "spectrum_dtype S48 needs n_doppler >= 64");
    if (c.mti_mode != FMCW_MTI_OFF || c.window == FMCW_WIN_Q15_RTL)
      return fail(FMCW_EINVAL, "spectrum_dtype S48 is defined with MTI off and an fp32 window (not Q15_RTL)");
  }
  if (c.spectrum_dtype == FMCW_SPEC_F16 && (c.compat_rtl & FMCW_COMPAT_MTI))
    return fail(FMCW_EINVAL, "compat MTI is defined on the fp32 spectrum (spectrum_dtype F16)");
  // the Q15 path rounds the corner-turned spectrum to int16 words (and windows them in K2): an fp16
  // spectrum has 11 significant bits, so words above 2048 would already be quantised
  if (c.spectrum_dtype == FMCW_SPEC_F16 && c.window == FMCW_WIN_Q15_RTL)
    return fail(FMCW_EINVAL, "window Q15_RTL is defined on the fp32 spectrum (spectrum_dtype F16)");
  return FMCW_OK;
}

int build_plan(const fmcw_config& c, const PlanPrefs& prefs, Plan* out) {
  Plan p{};
  p.cfg = c;
  // K1 family: k_range_px at N = 8192, the sequential-pair kernel at N = 4096, else k_range
  p.k1 = range_info(c.n_range, c.in_dtype, c.window, c.spectrum_dtype, prefs.k1_want);
  p.k1_stage = range_info(c.n_range, c.in_dtype, c.window, FMCW_SPEC_F32, prefs.k1_want);
  p.k2_fast = k2_fast(c) && !prefs.k2_generic;
  p.k2 = doppler_info(c.n_doppler, c.mti_mode, c.spectrum_dtype, p.k2_fast, false, p.k1.T);
  if (!p.k1.fn || !p.k2.fn)
    return fail(FMCW_EINVAL, "no kernel for this configuration (spectrum_dtype %d)", c.spectrum_dtype);
  // fmcw_range_ct launches k1_stage on k1's grid and un-tiles its output with k1's tile geometry
  if (p.k1_stage.T != p.k1.T || p.k1_stage.RB != p.k1.RB)
    return fail(FMCW_EINVAL, "stage K1 %s tiles %d x %d, path K1 %s %d x %d: fmcw_range_ct needs them equal",
                range_kind_name(p.k1_stage.kind), p.k1_stage.T, p.k1_stage.RB, range_kind_name(p.k1.kind), p.k1.T,
                p.k1.RB);
  p.lgT = __builtin_ctz(p.k1.T);
  p.lgRB = __builtin_ctz(p.k1.RB);
  p.tiles_frame = (int)(c.n_range / p.k2.WR);
  p.wpb = p.k2.NT / 64;
  p.cf1 = cfar1_args(c);
  if (c.cfar_kind == FMCW_CFAR_OS1D) p.cfar1 = cfar1_fn(c.n_doppler);
  p.frame_px = (size_t)c.n_range * c.n_doppler;
  p.in_frame_bytes = c.n_rx * p.frame_px * (c.in_dtype == FMCW_IN_F32 ? 8 : 4);
  p.frame_inter = c.n_rx * p.frame_px * (c.spectrum_dtype == FMCW_SPEC_F16   ? sizeof(uint32_t)
                                         : c.spectrum_dtype == FMCW_SPEC_S48 ? sizeof(S48)
                                                                             : sizeof(float2));
  p.q15 = c.window == FMCW_WIN_Q15_RTL;
  p.q15_scale = p.q15 ? std::ldexp(1.0f, -(int)c.range_shift) : 1.0f;
  p.chunk = chunk_frames(c, p.frame_inter);
  // >= one fp32 frame: fmcw_range_ct writes the fp32 spectrum through it whatever spectrum_dtype
  // (+16 B: an S48 point is read as the 8 bytes from its record rounded down to 4)
  p.inter_bytes = std::max((size_t)p.chunk * p.frame_inter, c.n_rx * p.frame_px * sizeof(float2)) + 16;
  if (c.cfar_kind == FMCW_CFAR_OS2D) {
    p.cf2 = cfar2_args(c);
    p.cfar2 = pick_cfar2(c, p.cf2);
    // candidate lists for K3 launches of up to k3_frames frames (fmcw_enqueue's batches: >= 16
    // frames, ending on a chunk boundary, so at most 16 + chunk - 1 frames): every cell may be a
    // candidate, so they cannot overflow.  8 B per cell: at 8192 x 1024 with the auto chunk (3
    // frames) 19 frames, 1.2 GiB.  A K3 launch addresses its cells with 32-bit indices, so
    // k3_frames is also capped at 2^32 cells (launch_cfar splits longer batches into pieces of
    // k3_frames).
    p.k3_frames = (int)std::max<size_t>(1, std::min<size_t>({(size_t)c.max_frames, kCfar2Batch + p.chunk,
                                                             (size_t)0xffffffffu / p.frame_px}));
    // K3 launches per call: one per chunk at most (map-less calls run it on each chunk's scratch),
    // else one per >= 16-frame batch, or one per k3_frames piece (fmcw_cfar)
    const size_t minb = std::min<size_t>(p.chunk, kCfar2Batch);
    p.k3_launches = (int)((c.max_frames + minb - 1) / minb + (c.max_frames + p.k3_frames - 1) / p.k3_frames + 2);
  }
  p.n_wg_max = (size_t)c.max_frames * p.tiles_frame;
  // Round 6 (verdict r5 item 1): by default (det_capacity 0) each wave tile owns a slot of ALL
  // its cells, so the detection count a call reports is always backed by stored records, det_cap
  // is the only bound on the list, and no tile ever takes an atomic to store its run -- the
  // reference emits every non-zero CFAR output (radar_core.vhd:413-418), and its own
  // cfar_scale_ovr = 1 (os_cfar_2d.vhd:191-192) detects ~25 % of Rayleigh cells.  Round 5's
  // scratch (slots of 1/32 of a tile, a shared overflow region of 1/64 of the cells) lost 21,199
  // of 86,735 records on a ::3 lattice, and its dense tiles serialised on the region's counter.
  // The memory (16 B per cell) is only reserved: untouched pages cost no bandwidth.  With
  // det_capacity N > 0 a slot holds 1/32 of its tile (32 entries for a 1024-cell tile) and a
  // denser tile moves its whole run to a shared overflow region of N records (one atomic per such
  // tile).
  const size_t cells_tile = p.frame_px / p.tiles_frame;
  p.slot_cap = (uint32_t)(c.det_capacity ? std::max<size_t>(32, cells_tile / 32) : cells_tile);
  const size_t slots = p.n_wg_max * p.slot_cap;
  const size_t cells = (size_t)c.max_frames * p.frame_px;
  const size_t ovf = c.det_capacity ? std::min<size_t>(c.det_capacity, cells) : 0;
  // 32-bit record indices; the overflow counter may run up to `cells` past ovf_base
  if (slots + cells >= 0xffffffffu)
    return fail(FMCW_EINVAL, "max_frames %u: %zu cells exceed the 2^32 detection records of one call",
                c.max_frames, cells);
  p.ovf_base = (uint32_t)slots;
  p.det_scratch_cap = (uint32_t)(slots + ovf);
  *out = p;
  return FMCW_OK;
}

}  // namespace fmcw
