/*
 * fmcw.h -- C-ABI of libfmcw.so, the MI355X (gfx950) FMCW range-Doppler + OS-CFAR
 * hot path.  Plain C types only: pointers, sizes, enums.  No torch, no C++.
 *
 * What this boundary replaces in the reference (Aurellia-Beam/fpga-fmcw-radar-processor):
 *
 *   fmcw_config            radar_core generics  rtl/src/radar_core.vhd:12-19 and control
 *                          ports mti_bypass / cfar_scale_ovr :47-49; FFT IP parameters
 *                          vivado_proj/.../ip/xfft_0_1/xfft_0.xci:12-27 (size, direction,
 *                          natural order); 1-D CFAR generics rtl/old/radar_core_v3.vhd:373-381
 *   fmcw_create            the FFT-IP config handshake cfg_proc radar_core.vhd:279-301
 *                          (config word x"0001" = forward, :247) -- done once per handle
 *   fmcw_enqueue /         the radar_core AXI4-Stream entity radar_core.vhd:21-56: ADC words
 *   fmcw_process           {Q[31:16], I[15:0]} in (:25-29), the Vivado IP calls
 *                          u_range_fft / u_doppler_fft (:303-316, :351-364) and every stage
 *                          between them (:267-390), detections out (:31-35, :396-418)
 *   fmcw_det               det_tdata[16:0] / det_range_bin[9:0] / det_doppler_bin[6:0]
 *                          (radar_core.vhd:31-35) + frame index + threshold (dbg_threshold,
 *                          rtl/src/os_cfar_2d.vhd:34, :219)
 *   status words 2, 3     the sticky status_overflow flag (radar_core.vhd:447-456), as counts:
 *   of fmcw_enqueue        samples saturated by the RTL-compat integer windows (win1 / win2
 *                          saturation, window_multiplier.vhd:152-158) and int16 spectrum words /
 *                          canceller outputs clipped (doppler_notch.vhd:75-93).  The fp32 build
 *                          spec never saturates; FMCW_EDETCAP reports a detection list overflow
 *   fmcw_range_ct          window_multiplier -> xfft_range -> corner_turner (:267-327),
 *                          corner-turned spectrum as the CT emits it (corner_turner.vhd:80)
 *   fmcw_magnitude         magnitude_calc (rtl/src/magnitude_calc.vhd:45-88)
 *   fmcw_cfar              os_cfar_2d / os_cfar on a caller-supplied magnitude map
 *                          (rtl/src/os_cfar_2d.vhd:83-230, rtl/old/os_cfar.vhd:98-137)
 *
 * Conventions
 *   - Return value: 0 (FMCW_OK) or a negative fmcw_status.  fmcw_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - fmcw_enqueue and the stage functions take DEVICE pointers only, are stream-ordered
 *     and asynchronous (nothing synchronises, nothing allocates).  fmcw_enqueue and fmcw_cfar
 *     can be captured into a hipGraph (stream capture) and the graph replayed any number of
 *     times, interleaved with direct calls on the same handle: the detection ordering pass keeps
 *     its call tag in device memory, and a captured call always re-zeroes the per-call counters
 *     first.  Replays of one handle's graphs must not overlap each other or other calls (one
 *     stream at a time, below); profiling (fmcw_set_profiling) must be off while capturing.
 *   - fmcw_process accepts host or device pointers (detected with hipPointerGetAttributes),
 *     and returns after the results are in the caller's buffers.
 *   - A handle is not thread-safe: one handle per host thread, and one stream at a time
 *     (its scratch -- intermediate spectrum, detection slots, counters -- is shared by its
 *     calls, so two calls in flight on different streams race).  Every entry point selects
 *     the handle's device itself.  All kernel scratch is allocated at fmcw_create for up to
 *     cfg.max_frames frames per call; fmcw_process keeps its host-copy staging in the handle.
 *   - Layouts (row-major, complex = interleaved re,im):
 *       cube   [frame][rx][chirp][sample]       in_dtype (f32 / f16 / int16 complex)
 *       map    [frame][range][doppler]          float32 (range-major, as radar_output.txt)
 *       spec   [frame][rx][range][chirp]        complex float32 (fmcw_range_ct)
 *     Doppler bin 0 is zero Doppler (natural FFT order, no fftshift).
 */
#ifndef FMCW_H_
#define FMCW_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMCW_ABI_VERSION 8  /* 2: fmcw_config grew compat_rtl, range_shift (27 words, 108 B);
                               3: + spectrum_dtype (28 words, 112 B);
                               4: FMCW_K_COUNT 5 -> 6, FMCW_INFO_PAIR_CHUNK;
                               5: n_dets_dev holds FMCW_STATUS_WORDS (4) words (saturation
                                  counts); the fused / paired kernels are gone (FMCW_K_COUNT 4,
                                  info keys 1-3 and 5 retired, fmcw_get_fused_trace removed);
                                  FMCW_WIN_Q15_RTL also windows slow time in integers;
                                  fmcw_comm_create takes wire_cap, fmcw_gather_dets det_cap;
                               6: fmcw_set_param (FMCW_PARAM_CFAR2D_STEPS), FMCW_INFO_CFAR2D_STEPS;
                                  range-kernel id 1 (k_range2) retired; the library reads no
                                  environment variable;
                               7: fmcw_enqueue / fmcw_cfar graph-capturable (device-resident
                                  ordering tag); fmcw_comm_fail_next_alloc_for_test,
                                  fmcw_comm_check_decide_for_test; FMCW_SPEC_S48;
                               8: fmcw_config grew det_capacity (29 words, 116 B): the detection
                                  scratch holds every cell by default, so a call loses no detection
                                  its det_cap has room for; fmcw_comm_info.
                               Still 8 with the plot extractor (fmcw_plots_*, fmcw_plot,
                               fmcw_plots_config): functions and types of its own were added, and
                               fmcw_config (29 words), FMCW_K_COUNT (4) and every existing
                               signature are unchanged.
                               Still 8 with the grid caps (FMCW_PARAM_GRID_*, FMCW_INFO_GRID_*) and
                               fmcw_plots_set_grid_for_test: new enum values and one new function,
                               no struct or signature change.
                               Still 8 with the bearing estimator (fmcw_bearings_*, fmcw_bearing,
                               fmcw_bearings_config): functions and types of its own, no existing
                               struct, enum or signature changes.
                               Still 8 with the beamformer (fmcw_beams_*, fmcw_beams_config):
                               functions and types of its own, nothing existing changes.
                               Still 8 with the cell-averaging detector (fmcw_cacfar_*,
                               fmcw_cacfar_config): functions and types of its own, nothing
                               existing changes.
                               Still 8 with the device tracker (fmcw_tws_dev_*, fmcw_tws_dev_config):
                               functions and types of its own; the host tracker fmcw_tws_* and every
                               existing struct, enum and signature are unchanged.
                               Still 8 with the clutter map (fmcw_cmap_*, fmcw_cmap_config): functions
                               and types of its own, nothing existing changes.
                               Still 8 with the adaptive beam weights (fmcw_adapt_*, fmcw_adapt_config)
                               and fmcw_beams_set_weights_dev: functions and types of their own; a
                               beamformer that never calls the new function behaves as before.
                               Still 8 with the beam merge (fmcw_merge_*, fmcw_mplot,
                               fmcw_merge_config): functions and types of its own, nothing
                               existing changes.
                               Still 8 with the velocity unfolder (fmcw_unfold_*, fmcw_vplot,
                               fmcw_unfold_config): functions and types of its own, nothing
                               existing changes.
                               Still 8 with the interference exciser (fmcw_excise_*,
                               fmcw_excise_config): functions and types of its own, in front of
                               fmcw_enqueue; nothing existing changes.
                               Still 8 with the TDM-MIMO virtual array (fmcw_mimo_*, fmcw_mimo_config):
                               functions and types of its own, between fmcw_range_ct and the objects
                               that read its spectrum; nothing existing changes.
                               Still 8 with the angle resolver (fmcw_doa_*, fmcw_doa, fmcw_doa_config):
                               functions and types of its own, behind fmcw_bearings_enqueue; nothing
                               existing changes */

typedef enum {
  FMCW_OK = 0,
  FMCW_EINVAL = -1,       /* bad argument / unsupported configuration */
  FMCW_ENOMEM = -2,       /* device allocation failed */
  FMCW_EHIP = -3,         /* HIP runtime error (message in fmcw_last_error) */
  FMCW_EDETCAP = -4,      /* detection list longer than det_cap; *n_dets = required count */
  FMCW_ENODEV = -5        /* no usable gfx950 device */
} fmcw_status;

typedef enum { FMCW_IN_F32 = 0, FMCW_IN_F16 = 1, FMCW_IN_I16 = 2 } fmcw_in_dtype;
/* FMCW_WIN_Q15_RTL (RTL-compat, in_dtype I16 only): both windows in the RTL's integer
 * arithmetic, y = sat16((x * c[n] + 2^14) >> 14) with the ROM c = round(32767 w) on the
 * mirrored half address (window_multiplier.vhd:43-46, :97-102, :146-158) -- a 2x gain with a
 * +1 LSB bias, so a zero word windows to 1.  Fast time: on the ADC words (u_range_window,
 * radar_core.vhd:267-276).  Slow time (u_doppler_window, :340-349): on the corner-turned
 * spectrum's 16-bit words -- the range spectrum scaled by 2^-range_shift (the IP's fixed
 * scaling schedule; pick range_shift so it fits 16 bits), rounded half-to-even and saturated
 * to int16 -- after the MTI canceller when it is on.  The FFTs stay unscaled fp32.  Saturated
 * samples are counted in status words 2 (windows) and 3 (spectrum words, canceller). */
typedef enum { FMCW_WIN_NONE = 0, FMCW_WIN_HAMMING = 1, FMCW_WIN_Q15_RTL = 2 } fmcw_window;
/* FMCW_MAG_ABS: |X| = sqrt(re^2 + im^2) (with n_rx > 1: sqrt(sum_rx |X_rx|^2), NCI).
 * FMCW_MAG_AMBM: max(|re|,|im|) + floor(min/4) + floor(min/8) (magnitude_calc.vhd:78-81). */
typedef enum { FMCW_MAG_ABS = 0, FMCW_MAG_AMBM = 1 } fmcw_mag_mode;
/* What fmcw_enqueue writes into rd_map: linear magnitude, or 20*log10(mag + 1). */
typedef enum { FMCW_MAP_LINEAR = 1, FMCW_MAP_DB = 2 } fmcw_map_kind;
typedef enum { FMCW_CFAR_NONE = 0, FMCW_CFAR_OS1D = 1, FMCW_CFAR_OS2D = 2 } fmcw_cfar_kind;
/* MTI / Doppler notch on the corner-turned spectrum, along slow time per range bin, delay
 * line zeroed at each range bin's first chirp (rtl/src/doppler_notch.vhd:72-102):
 * 2-pulse y[c] = x[c] - x[c-1];  3-pulse y[c] = x[c] - 2 x[c-1] + x[c-2].  OFF = bypass. */
typedef enum { FMCW_MTI_OFF = 0, FMCW_MTI_2PULSE = 2, FMCW_MTI_3PULSE = 3 } fmcw_mti_mode;

typedef struct fmcw_config {
  uint32_t n_range;        /* Ns: samples per chirp = range bins (N_RANGE); power of 2, 64..8192 */
  uint32_t n_doppler;      /* Nc: chirps per frame = Doppler bins (N_DOPPLER); power of 2, 32..1024 */
  uint32_t n_rx;           /* receive channels, >= 1; > 1 => non-coherent integration */
  int32_t in_dtype;        /* fmcw_in_dtype */
  int32_t window;          /* fmcw_window, applied on both fast and slow time */
  int32_t mag_mode;        /* fmcw_mag_mode */
  int32_t map_kind;        /* fmcw_map_kind */
  int32_t cfar_kind;       /* fmcw_cfar_kind */
  int32_t mti_mode;        /* fmcw_mti_mode (mti_bypass port, radar_core.vhd:48) */
  /* 1-D OS-CFAR along Doppler (circular): rtl/old/os_cfar.vhd generics */
  uint32_t cfar1d_ref;     /* reference cells per side (REF_CELLS, 8) */
  uint32_t cfar1d_guard;   /* guard cells per side (GUARD_CELLS, 2) */
  uint32_t cfar1d_rank;    /* 0-based ascending rank k (RANK_IDX, 12) */
  float cfar1d_alpha;      /* threshold multiplier (SCALING_MULT/SCALING_DIV, 4) */
  /* 2-D OS-CFAR (rtl/src/os_cfar_2d.vhd), named by the axis each acts on (the RTL's
   * GUARD_RANGE=2 acts along Doppler, GUARD_DOPPLER=1 along range) */
  uint32_t cfar2d_ref_range;      /* 4 */
  uint32_t cfar2d_guard_range;    /* 1 */
  uint32_t cfar2d_ref_doppler;    /* 4 */
  uint32_t cfar2d_guard_doppler;  /* 2 */
  uint32_t cfar2d_rank_pct;       /* RANK_PCT 75 -> k = floor(n_ref*pct/100) */
  uint32_t cfar2d_scale_min;      /* SCALE_MIN 2 */
  uint32_t cfar2d_scale_nom;      /* SCALE_NOM 4 */
  uint32_t cfar2d_scale_max;      /* SCALE_MAX 6 */
  uint32_t cfar2d_scale_override; /* cfar_scale_ovr port; 0 = adaptive */
  /* resources */
  uint32_t max_frames;     /* largest n_frames per call (scratch is sized for it) */
  uint32_t chunk_frames;   /* frames per internal kernel chunk (0 = auto: a chunk's corner-turned
                            * spectrum within 208 MiB of the 256 MiB Infinity Cache, no rounding;
                            * 104 frames at 1024 x 256 fp32, 3 at 4096 x 512 x 4 rx or 8192 x 1024).
                            * Device memory of a handle: the chunk's spectrum (8 B per point), the
                            * detection scratch (det_capacity below: 16 B per record), and with the
                            * 2-D CFAR a chunk-sized linear map (4 B per cell) and candidate lists of
                            * 8 B per cell for min(max_frames, 16 + chunk, 2^32 cells) frames --
                            * 1.2 GiB at 8192 x 1024 with the auto chunk */
  int32_t device_id;       /* HIP device ordinal */
  /* RTL-compat arithmetic, a bitmask of fmcw_compat; 0 = the fp32 build spec */
  uint32_t compat_rtl;
  /* range FFT output scaled by 2^-range_shift (exact): the Xilinx IP's fixed scaling schedule
   * SCALE_SCH (tb_xfft_128.vhd:480-494), so that spectra fit the IP's 16-bit output word;
   * 0..13 */
  uint32_t range_shift;
  /* fmcw_spectrum_dtype: element type of the internal corner-turned spectrum */
  int32_t spectrum_dtype;
  /* Detection records the handle's scratch holds for one call.  0 (default): a slot of every
   * cell of each detection tile (16 B per cell of max_frames frames: 4 GiB at 1024 frames of
   * 1024 x 256), so no call can lose a detection at any density the CFAR parameters produce --
   * the reference emits every non-zero CFAR output (radar_core.vhd:413-418), and cfar_scale_ovr
   * = 1 or a 1-D alpha of 1 detect ~25 % of noise cells.  N > 0, for callers that bound det_cap:
   * slots of 1/32 of a tile's cells plus a shared region of N records for denser tiles; a call
   * then loses records (status word [1]) only when it finds more than N detections, i.e. never
   * while det_cap <= N would have room for the whole list.  max_frames x cells must stay below
   * 2^32 records. */
  uint32_t det_capacity;
} fmcw_config;

/* fmcw_config.spectrum_dtype.  FMCW_SPEC_F16 stores the corner-turned spectrum (K1 -> K2) as
 * fp16 pairs holding X / n_range: 4 instead of 8 bytes per point written and read back
 * (config 5: 160 -> 128 MiB of HBM traffic per frame).  The map then carries fp16 rounding of
 * the range spectrum: max |map - oracle| <= 2e-3 x max|oracle| per frame (tested), against
 * 1e-4 for FMCW_SPEC_F32; detections stay bit-exact to the oracle CFAR on the map produced.
 * Not with FMCW_COMPAT_MTI (its 16-bit words are defined on the fp32 spectrum).
 * FMCW_SPEC_S48 stores it in 6 bytes per point (config 2: 2 -> 1.5 MiB written and read back per
 * frame; configs 3 / 5: 64 -> 48 MiB, so the auto chunk holds 4 frames instead of 3): a group of
 * G chirps of a range bin (adjacent quads at n_range <= 512; chirps n_doppler / 16 apart at
 * n_range = 1024 (quads) and above (pairs)) shares one 8-bit exponent E (the largest of their 2G components is
 * < 2^E), and every component is a W-bit signed significand of 2^(E - W + 1), i.e. exact to 2^-W
 * of the group's largest component (fp32: 2^-24 of each) -- G = 4, W = 23 at n_range <= 1024;
 * G = 2, W = 22 above.  The map stays within the 1e-4 tolerance of FMCW_SPEC_F32 (per frame and
 * per bin above 1e-3 of the frame peak; tested).  Needs n_doppler >= 64, MTI off and a fp32
 * window. */
typedef enum { FMCW_SPEC_F32 = 0, FMCW_SPEC_F16 = 1, FMCW_SPEC_S48 = 2 } fmcw_spectrum_dtype;

/* fmcw_config.compat_rtl bits.
 * FMCW_COMPAT_CFAR: the CFAR on the RTL's 17-bit unsigned cells (DATA_WIDTH 17): each map
 *   cell enters the CFAR as q = min(floor(max(x, 0)), 2^17 - 1) (the map itself is unchanged).
 *   1-D (rtl/old/os_cfar.vhd:132-137): T = (ranked * alpha) mod 2^17 (resize to DATA_WIDTH),
 *   detect q_cut > T; alpha must be an integer (SCALING_MULT, SCALING_DIV = 1).
 *   2-D (rtl/src/os_cfar_2d.vhd:163, :189-213): mean = floor(sum / n_ref) of the integer refs,
 *   hi = (mean + (mean >> 1)) mod 2^17 (a 17-bit add), lo = mean >> 1, the same brackets,
 *   T = ranked * scale at full width.  fmcw_det.mag / .threshold carry q_cut and T.
 * FMCW_COMPAT_MTI: the MTI canceller on 16-bit words (rtl/src/doppler_notch.vhd:67-93): the
 *   (range_shift-scaled) spectrum is rounded half-to-even and saturated to int16 (the IP's
 *   output word, convergent rounding xfft_0.xci), then y = sat16(x - x1) or
 *   sat16(x - 2 x1 + x2) in integers.  Needs mti_mode != OFF. */
typedef enum { FMCW_COMPAT_CFAR = 1, FMCW_COMPAT_MTI = 2 } fmcw_compat;

/* One detection: 16 bytes, sorted by (frame, range, doppler). */
typedef struct fmcw_det {
  uint32_t frame;
  uint16_t range;
  uint16_t doppler;
  float mag;        /* CUT magnitude (det_tdata) */
  float threshold;  /* scale * ranked reference cell (dbg_threshold) */
} fmcw_det;

typedef struct fmcw_handle fmcw_handle;

/* Kernel ids for fmcw_kernel_times (profiling). */
typedef enum {
  FMCW_K_RANGE = 0,   /* window + range FFT + corner turn */
  FMCW_K_DOPPLER = 1, /* Doppler window + FFT + magnitude (+NCI) (+1-D CFAR) + map */
  FMCW_K_CFAR2D = 2,  /* 2-D OS-CFAR */
  FMCW_K_COMPACT = 3, /* detection list ordering */
  FMCW_K_COUNT = 4
} fmcw_kernel_id;

/* fmcw_get_info keys.  FMCW_INFO_CHUNK: frames per K1 -> K2 chunk.  FMCW_INFO_RANGE_KERNEL: the
 * range-stage kernel the handle runs: 0 k_range (T chirps per workgroup; every N, and the Q15 /
 * fp16-spectrum paths), 2 k_range_sq (two chirps one after the other through one chirp's LDS;
 * N = 4096), 3 k_range_px (as 2 with two LDS exchanges and a cross-lane last pass; N = 8192);
 * 1 (round 2's k_range2) is retired.  FMCW_INFO_WINDOW_SATURATIONS / FMCW_INFO_WORD_SATURATIONS:
 * status words 2 / 3 of the last fmcw_process call (fmcw_enqueue callers read them from
 * n_dets_dev).  FMCW_INFO_CFAR2D_STEPS: the strip length (workgroup steps) of the handle's last
 * 2-D CFAR launch (0 before the first).  FMCW_INFO_GRID_*: the handle's current bound on the
 * workgroups of a persistent kernel (the FMCW_PARAM_GRID_* of the same name below): the grid
 * computed at fmcw_create, or the cap set since.  A launch uses the smaller of this bound and its
 * own unit count. */
typedef enum { FMCW_INFO_CHUNK = 4, FMCW_INFO_RANGE_KERNEL = 6, FMCW_INFO_WINDOW_SATURATIONS = 7,
               FMCW_INFO_WORD_SATURATIONS = 8, FMCW_INFO_CFAR2D_STEPS = 9,
               FMCW_INFO_GRID_RANGE = 10, FMCW_INFO_GRID_DOPPLER = 11, FMCW_INFO_GRID_CFAR2D = 12,
               FMCW_INFO_GRID_K3B = 13, FMCW_INFO_GRID_K3C = 14 } fmcw_info_key;

/* fmcw_set_param keys (tuning; results never depend on them).  FMCW_PARAM_CFAR2D_STEPS: steps
 * (4-wave-tile workgroup tiles) per 2-D CFAR strip, 0 = the library's cost model (default).
 * FMCW_PARAM_GRID_*: a cap on the workgroups of a persistent kernel, whose workgroups stride over
 * their units whatever the grid: _RANGE the range stage (K1), _DOPPLER the Doppler stage (K2) and the
 * stand-alone 1-D CFAR, _CFAR2D / _K3B / _K3C the three kernels of the 2-D CFAR.  Value 0 restores
 * the grid computed at fmcw_create (occupancy x compute units; fixed grids for K3B / K3C), 1..2^20
 * sets min(that grid, value); anything else is FMCW_EINVAL.  Fewer workgroups leave compute units
 * to other streams' kernels.  The key and the value are checked before the handle.  A captured
 * graph keeps the grids it was captured with: a cap set afterwards reaches only later calls and
 * captures. */
typedef enum { FMCW_PARAM_CFAR2D_STEPS = 1, FMCW_PARAM_GRID_RANGE = 2, FMCW_PARAM_GRID_DOPPLER = 3,
               FMCW_PARAM_GRID_CFAR2D = 4, FMCW_PARAM_GRID_K3B = 5, FMCW_PARAM_GRID_K3C = 6 } fmcw_param_key;

/* Status words of fmcw_enqueue / fmcw_cfar (n_dets_dev). */
#define FMCW_STATUS_WORDS 4

/* Only the functions below are exported from libfmcw.so (built -fvisibility=hidden). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

const char* fmcw_version(void);
int fmcw_abi_version(void);
const char* fmcw_last_error(void);

/* Defaults = the reference core: N_RANGE 1024, N_DOPPLER 128, 1 rx, f32 in, Hamming,
 * |X|, linear map, 2-D OS-CFAR with radar_core.vhd:376-382 parameters. */
void fmcw_config_default(fmcw_config* cfg);

int fmcw_create(const fmcw_config* cfg, fmcw_handle** out);
int fmcw_destroy(fmcw_handle* h);

/* Full hot path on n_frames frames, device pointers, asynchronous on `stream`
 * (hipStream_t; NULL = default stream).  rd_map may be NULL.  dets may be NULL when
 * cfar_kind == NONE.  n_dets_dev points at FMCW_STATUS_WORDS device uint32 words, written by
 * the last kernel of every call that returns FMCW_OK (a call that returns an error may have
 * left them as the previous call wrote them); it may be NULL only when cfar_kind == NONE (then
 * no status):
 *   [0] detections found (may exceed det_cap; entries beyond det_cap are not written),
 *   [1] detections lost because the handle's detection scratch overflowed: only possible with
 *       cfg.det_capacity = N > 0 and more than N detections found (the default scratch holds
 *       every cell).  Non-zero means the list is incomplete; fmcw_process returns FMCW_EDETCAP
 *       then.  0xffffffff: the ordering pass could not complete (a safety net that bounds its
 *       wait; not expected), the whole list is void,
 *   [2] samples saturated by the RTL-compat integer windows (FMCW_WIN_Q15_RTL, either axis;
 *       win1 / win2 saturation_flag, window_multiplier.vhd:152-158),
 *   [3] samples whose int16 spectrum word or canceller output was clipped (FMCW_COMPAT_MTI or
 *       FMCW_WIN_Q15_RTL; doppler_notch.vhd:75-93).
 * [2] and [3] stay 0 on the fp32 build spec, which cannot saturate. */
int fmcw_enqueue(fmcw_handle* h, const void* cube, size_t n_frames, float* rd_map,
                 fmcw_det* dets, size_t det_cap, uint32_t* n_dets_dev, void* stream);

/* Synchronous convenience wrapper; pointers may be host or device memory. */
int fmcw_process(fmcw_handle* h, const void* cube, size_t n_frames, float* rd_map,
                 fmcw_det* dets, size_t det_cap, size_t* n_dets, void* stream);

/* Stage entry points (device pointers, asynchronous).
 * fmcw_cfar reads the map as the RTL's unsigned magnitude stream (magnitude_calc.vhd:45-88):
 * negative cells and -0.0 are taken as +0.  NaN cells are outside the specification (the RTL's
 * magnitudes are integers, and the sorting and counting forms of the OS-CFAR disagree on NaN):
 * a NaN reference never counts, and the 2-D CFAR's level screens (the reference window) take a
 * NaN CUT as below every level and screen it out, so whether a NaN CUT is reported is not
 * specified.  +Inf cells are supported. */
int fmcw_range_ct(fmcw_handle* h, const void* cube, size_t n_frames, void* spec, void* stream);
int fmcw_magnitude(const float* iq, float* out, size_t n, int mag_mode, void* stream);
int fmcw_cfar(fmcw_handle* h, const float* map, size_t n_frames, fmcw_det* dets,
              size_t det_cap, uint32_t* n_dets_dev, void* stream);

/* ---- Multi-GPU detection gather (RCCL over xGMI) ------------------------
 * The reference is one FPGA and has no distributed layer; this is the optional gather of
 * frame-sharded detection lists to one root rank.  One process per GPU.  Rank 0 makes the
 * id (fmcw_comm_unique_id), the caller distributes its FMCW_COMM_ID_BYTES bytes out of band,
 * every rank calls fmcw_comm_create (collective) with the SAME wire_cap (record slots per
 * rank message, 1..2^26; checked with one all-reduce there: FMCW_EINVAL if the ranks differ).
 * fmcw_gather_dets is stream-ordered, allocates nothing and never synchronises with the host:
 * every rank sends a fixed-size message (a 16-B header holding its count, then wire_cap record
 * slots) to `root` with ncclSend/ncclRecv, and the root compacts the lists on the device in
 * rank order (= global frame order for contiguous shards).  A rank sends min(n_dets_dev[0],
 * det_cap, wire_cap) records of dets_dev (det_cap = the capacity of dets_dev, as passed to
 * fmcw_enqueue), each .frame plus `frame_offset` (its first global frame).  On the root:
 * out_dev holds n_ranks * wire_cap records, out_n_dev[0] = records written, out_n_dev[1] =
 * records not sent (beyond det_cap or wire_cap, plus the ranks' n_dets_dev[1] scratch
 * losses).  Other ranks may pass NULL out pointers. */
#define FMCW_COMM_ID_BYTES 128
typedef struct fmcw_comm fmcw_comm;
int fmcw_comm_unique_id(void* id_out);
int fmcw_comm_create(const void* id, int n_ranks, int rank, int device_id, size_t wire_cap,
                     fmcw_comm** out);
int fmcw_comm_destroy(fmcw_comm* c);
/* What RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank /
 * ncclCommCuDevice), so that a multi-GPU run can show the collective really spans n_ranks GPUs;
 * wire_cap as created.  Any output pointer may be NULL. */
int fmcw_comm_info(const fmcw_comm* c, int* n_ranks, int* rank, int* device, size_t* wire_cap);
int fmcw_gather_dets(fmcw_comm* c, const fmcw_det* dets_dev, size_t det_cap,
                     const uint32_t* n_dets_dev, uint32_t frame_offset, fmcw_det* out_dev,
                     uint32_t* out_n_dev, int root, void* stream);
/* Test hooks of fmcw_comm_create's failure handling: fail_next_alloc makes the process's next
 * fmcw_comm_create treat its buffer allocation as failed (after ncclCommInitRank, before the
 * collective check, which every rank joins whatever failed locally); check_decide returns that
 * check's verdict on the all-reduced words h[3] = max over ranks of {wire_cap, ~wire_cap, failed}
 * (FMCW_ENOMEM if any rank failed, FMCW_EINVAL if wire_cap differs, else FMCW_OK). */
int fmcw_comm_fail_next_alloc_for_test(int enable);
int fmcw_comm_check_decide_for_test(const uint64_t* h, int local_fail, size_t wire_cap);
/* Single-GPU test hooks of the gather's device side (no RCCL): the rank-local pack into one
 * message of (1 + wire_cap) records, and the root's compaction of n_ranks such messages laid
 * end to end in msgs_dev. */
int fmcw_gather_pack_for_test(const fmcw_det* dets_dev, size_t det_cap, const uint32_t* n_dets_dev,
                              size_t wire_cap, uint32_t frame_offset, fmcw_det* msg_dev, void* stream);
int fmcw_gather_compact_for_test(const fmcw_det* msgs_dev, int n_ranks, size_t wire_cap,
                                 fmcw_det* out_dev, uint32_t* out_n_dev, void* stream);

/* Profiling: when enabled, every stage launch carries hipEvents on its stream that take the
 * dispatches' own begin / end timestamps (hipExtLaunchKernelGGL: the first launch of a stage
 * starts the event pair, its last one stops it); fmcw_kernel_times synchronises and returns, per
 * fmcw_kernel_id, the summed milliseconds and the number of stage launches since the last reset. */
int fmcw_set_profiling(fmcw_handle* h, int enable);
int fmcw_set_param(fmcw_handle* h, int key, int64_t value);
int fmcw_get_info(fmcw_handle* h, int key, int64_t* value);
int fmcw_kernel_times(fmcw_handle* h, double* ms, uint64_t* launches);
int fmcw_reset_kernel_times(fmcw_handle* h);

/* Scratch-free helpers so callers without a device allocator can use the library. */
int fmcw_device_alloc(size_t bytes, void** ptr, int device_id);
int fmcw_device_free(void* ptr);
int fmcw_memcpy(void* dst, const void* src, size_t bytes, int kind /*0 H2D,1 D2H,2 D2D*/);
int fmcw_device_count(int* n);

/* ---- Plot extraction (peak grouping) between the CFAR and the tracker -------------------
 * The reference streams every CFAR output into tws_tracker (radar_core.vhd:413-438), which keeps
 * a scan's first MAX_DETS = 64; a point target's main lobe and sidelobes are dozens of detections,
 * so those slots go to the nearest target's cells.  The plotter turns the detection list into one
 * fmcw_plot per local maximum, on the device, from the list alone (no map).  It is an object of
 * its own, not part of fmcw_handle / fmcw_config.
 *
 * Input: a detection list as fmcw_enqueue / fmcw_cfar write it (records strictly increasing in
 * (frame, range, doppler), range < n_range, doppler < n_doppler) and its count word.
 * The window of a detection P = (f, r, d) is every detection (f, r + dr, (d + dd) mod n_doppler)
 * of the same frame with |dr| <= win_range, |dd| <= win_doppler and 0 <= r + dr < n_range:
 * Doppler is circular, range is clamped, P is in its own window.  P is a peak iff for every other
 * Q of its window mag(P) > mag(Q), or mag(P) == mag(Q) and P precedes Q in the list.  Every peak
 * gives one plot, in list order of the peaks.  NaN magnitudes are outside the specification. */
typedef struct fmcw_plot {   /* 32 bytes */
  uint32_t frame;
  uint16_t range;            /* the peak cell */
  uint16_t doppler;
  float mag;                 /* the peak's record, bit for bit */
  float threshold;
  uint32_t n_cells;          /* detections in the window, the peak included */
  float sum_mag;             /* S = sum of their mag (fp32, rows in ascending dr) */
  float d_range;             /* sum(mag * dr) / S: centroid offset from the peak cell in bins, */
  float d_doppler;           /* sum(mag * dd) / S; |.| <= win; both 0 if S is 0 or not finite */
} fmcw_plot;
typedef struct fmcw_plots_config {   /* 24 bytes */
  uint32_t n_range;          /* 1..65536 */
  uint32_t n_doppler;        /* 2 win_doppler + 1 .. 65536 */
  uint32_t win_range;        /* 0..4 */
  uint32_t win_doppler;      /* 0..4 */
  uint32_t max_dets;         /* most records one call examines, 1..2^31-1; scratch: 1 bit per record
                                and 4 B per 1024 records */
  int32_t device_id;         /* 0..63 */
} fmcw_plots_config;
typedef struct fmcw_plotter fmcw_plotter;
/* Status words of fmcw_plots_enqueue (n_plots_dev). */
#define FMCW_PLOT_STATUS_WORDS 2
/* Defaults: 1024, 128, window 1 x 1, max_dets 2^20, device 0. */
void fmcw_plots_config_default(fmcw_plots_config* cfg);
/* Validates before any device access (FMCW_EINVAL, the message names the field), then
 * FMCW_ENODEV / FMCW_ENOMEM as fmcw_create.  Allocates all scratch. */
int fmcw_plots_create(const fmcw_plots_config* cfg, fmcw_plotter** out);
int fmcw_plots_destroy(fmcw_plotter* p);   /* NULL is FMCW_OK */
/* Device pointers only; stream-ordered, allocates nothing, never synchronises, and keeps no state
 * between calls, so it can be captured into a hipGraph after fmcw_enqueue on the same stream and
 * replayed.  One stream at a time per plotter (its scratch is shared by its calls).
 * Examines n = min(n_dets_dev[0], det_cap, max_dets) records (n is read on the device) and writes
 * FMCW_PLOT_STATUS_WORDS words:
 *   n_plots_dev[0] plots found (may exceed plot_cap: then the first plot_cap plots are written and
 *                  nothing is stored beyond them),
 *   n_plots_dev[1] n_dets_dev[0] - n, the records not examined.
 * With n = 0 it writes {0, n_dets_dev[0]} and touches no plot. */
int fmcw_plots_enqueue(fmcw_plotter* p, const fmcw_det* dets_dev, size_t det_cap,
                       const uint32_t* n_dets_dev, fmcw_plot* plots_dev, size_t plot_cap,
                       uint32_t* n_plots_dev, void* stream);
/* Test hook: bounds the workgroups of the plotter's two tile kernels (find, emit), which stride
 * over the 1024-record tiles, so that a short list drives a workgroup through several tiles.
 * 0 = the built-in bound (4096), else min(that bound, grid).  Plots never depend on it. */
int fmcw_plots_set_grid_for_test(fmcw_plotter* p, uint32_t grid);

/* ---- Beam merge: one report per target across the beams of a scan, with beam position ----
 * After the beamformer the chain runs on n_frames * n_beams maps, and a record's .frame is
 * m = f * n_beams + b (scan f, beam b).  Neighbouring beams overlap, so one target gives a plot in
 * every beam that sees it.  The merger is the plot extractor's peak grouping with the beam as a
 * third axis: a record list in, one fmcw_mplot per local maximum over (beam, range, Doppler) out,
 * on the device, from the list alone.  It is an object of its own, not part of fmcw_handle.
 *
 * Input: a record list and its count word.  A record begins {uint32 frame; uint16 range; uint16
 * doppler; float mag}; the stride is 16 (fmcw_det) or 32 (fmcw_plot).  Records are strictly
 * increasing in (frame, range, doppler), range < n_range, doppler < n_doppler.  Record frame m is
 * scan f = m / n_beams, beam b = m % n_beams.
 * The neighbourhood of P = (f, b, r, d) is every record (f, b + db, r + dr, (d + dd) mod n_doppler),
 * P included, with |db| <= win_beam, |dr| <= win_range, |dd| <= win_doppler and 0 <= r + dr <
 * n_range; the beam axis is clamped (0 <= b + db < n_beams) when beam_wrap == 0 and circular
 * ((b + db) mod n_beams; DFT beams, whose u axis wraps) when beam_wrap == 1, which requires
 * n_beams >= 2 win_beam + 1.  Doppler is circular, range is clamped.  P is a peak iff for every
 * other Q of its neighbourhood mag(P) > mag(Q), or mag(P) == mag(Q) and P precedes Q in the list.
 * Every peak gives one merged plot, in list order of the peaks, so the output's .frame (the scan)
 * is non-decreasing, as the device tracker requires.  NaN magnitudes are outside the
 * specification. */
typedef struct fmcw_mplot {   /* 32 bytes: fmcw_tws_dev_enqueue and fmcw_bearings_enqueue take it at stride 32 */
  uint32_t frame;            /* the scan f (not f * n_beams + b) */
  uint16_t range;            /* the peak record's cell */
  uint16_t doppler;
  float mag;                 /* the peak record's mag, bit for bit */
  uint16_t beam;             /* the peak's beam */
  uint16_t n_merged;         /* records in the neighbourhood, the peak included (<= 729) */
  float sum_mag;             /* S = sum of their mag (fp32; ascending db, then dr, then the column runs) */
  float d_beam;              /* sum(mag * db) / S: offsets from the peak in beams / bins; on a wrapped */
  float d_range;             /* sum(mag * dr) / S  beam axis db is the signed offset in [-win_beam,    */
  float d_doppler;           /* sum(mag * dd) / S  win_beam]; |.| <= win; all 0 if S is 0 or not finite */
} fmcw_mplot;
typedef struct fmcw_merge_config {   /* 10 words, 40 bytes */
  uint32_t n_range;          /* 1..65536 */
  uint32_t n_doppler;        /* 2 win_doppler + 1 .. 65536 */
  uint32_t n_beams;          /* 1..64 */
  uint32_t win_beam;         /* 0..4 */
  uint32_t win_range;        /* 0..4 */
  uint32_t win_doppler;      /* 0..4 */
  uint32_t beam_wrap;        /* 0: beam axis clamped; 1: circular (n_beams >= 2 win_beam + 1) */
  uint32_t max_recs;         /* most records one call examines, 1..2^31-1; scratch: 1 bit per record
                                and 4 B per 1024 records */
  uint32_t max_maps;         /* most maps (scans * n_beams) one call covers: >= n_beams, a multiple of
                                it, < 2^31; scratch: 4 B per map */
  int32_t device_id;         /* 0..63 */
} fmcw_merge_config;
typedef struct fmcw_merger fmcw_merger;
/* Status words of fmcw_merge_enqueue (status_dev). */
#define FMCW_MERGE_STATUS_WORDS 3
/* Defaults: 1024, 128, 1 beam, windows 1 / 1 / 1, no wrap, max_recs 2^20, max_maps 1024, device 0. */
void fmcw_merge_config_default(fmcw_merge_config* cfg);
/* Validates every field before any device access (FMCW_EINVAL, the message names the field), then
 * FMCW_ENODEV / FMCW_ENOMEM as fmcw_plots_create.  Allocates all scratch. */
int fmcw_merge_create(const fmcw_merge_config* cfg, fmcw_merger** out);
int fmcw_merge_destroy(fmcw_merger* m);   /* NULL is FMCW_OK */
/* Device pointers only; stream-ordered, allocates nothing, never synchronises, uses no atomic and
 * keeps no state between calls: every word a later launch reads is written by an earlier launch of
 * the same call, so it can be captured into a hipGraph (after fmcw_plots_enqueue, say) and replayed.
 * One stream at a time per merger.  rec_stride is 16 or 32; recs_dev and out_dev are 16-byte
 * aligned; n_maps <= max_maps and a multiple of n_beams (FMCW_EINVAL otherwise, before any device
 * access).  Examines n = min(n_recs_dev[0], rec_cap, max_recs) records (n is read on the device) and
 * writes FMCW_MERGE_STATUS_WORDS words:
 *   status_dev[0] merged plots found (may exceed out_cap: then the first out_cap are written and
 *                 nothing is stored beyond them),
 *   status_dev[1] n_recs_dev[0] - n, the records not examined,
 *   status_dev[2] the examined records whose frame >= n_maps.  They form a suffix and are ignored:
 *                 never a peak, never a neighbour, and no memory is indexed by them.
 * With n = 0 it writes {0, n_recs_dev[0], 0} and touches nothing else. */
int fmcw_merge_enqueue(fmcw_merger* m, const void* recs_dev, size_t rec_stride, size_t rec_cap,
                       const uint32_t* n_recs_dev, size_t n_maps, fmcw_mplot* out_dev, size_t out_cap,
                       uint32_t* status_dev, void* stream);
/* Test hook: bounds the workgroups of the merger's tile kernels (index, find, emit), which stride
 * over 1024-record tiles.  0 = the built-in bound (4096), else min(that bound, grid).  Merged plots
 * never depend on it. */
int fmcw_merge_set_grid_for_test(fmcw_merger* m, uint32_t grid);

/* ---- Velocity unfolding: one report per target and dwell across a PRF stagger ------------
 * A staggered radar changes its PRF from scan to scan, because one PRF folds a fast target's
 * Doppler onto the wrong bin (and at a blind speed onto bin 0, where the canceller removes it).
 * The unfolder turns every dwell of K staggered scans into one report per target with its
 * unambiguous radial velocity, on a Doppler axis that is the same for every PRF.  A record list in,
 * a record list out, on the device, from the lists alone; an object of its own, not part of
 * fmcw_handle.
 *
 * Units.  PRF k (k = 0 .. n_prf - 1) is prf_units[k] * f0 = p_k f0 for a common f0.  The fine unit
 * of frequency is f0 / n_doppler, so one Doppler bin of PRF k is p_k fine units.
 * Input: a record list and its count word.  A record begins {uint32 frame; uint16 range; uint16
 * doppler; float mag}; the stride is 16 (fmcw_det) or 32 (fmcw_plot, fmcw_mplot).  Records are
 * strictly increasing in (frame, range, doppler).  Record frame m is scan s = m / n_streams of
 * stream t = m % n_streams, as fmcw_tws_dev_enqueue reads it; streams never interact.  Scan s uses
 * PRF index (s + prf_phase) % n_prf.  Dwell j covers scans j step .. j step + K - 1 (K = n_prf);
 * there are n_dwells = (n_scans - K) / step + 1 of them, none if n_scans < K.
 *
 * A record P = (scan s, stream t, r, d, mag) belongs to every dwell j that contains s, at position
 * i = s - j step, with PRF index k.  With Nc = n_doppler and all integers exact:
 *   1. ds = (d - zero_bin) mod Nc, minus Nc if ds >= (Nc + 1) / 2;
 *   2. the hypotheses are v_m = (ds + m Nc) p_k for every integer m with |v_m| <= v_max, ascending m;
 *   3. at another position i' (scan s', PRF index k') v_m predicts the bin
 *      d' = (floor((2 v_m + p_k') / (2 p_k')) + zero_bin) mod Nc;
 *   4. position i' is a hit if stream t's scan s' holds a record (r + dr, (d' + dd) mod Nc) with
 *      |dr| <= tol_range, 0 <= r + dr < n_range, |dd| <= tol_doppler; the hit's record is the one of
 *      largest mag in that window, the first in list order among equals; P's own position is always a
 *      hit, with P as its record;
 *   5. the best hypothesis has the most hits, then the smaller |v|, then the smaller m; n_ties counts
 *      the hypotheses that share the best hit count;
 *   6. P reports in dwell j iff the best hypothesis has at least m_of hits and none of them at a
 *      position before i: the earliest scan that sees the target owns the report.
 * Reports come out in the order (dwell j, stream t, list order of P within that stream's scans of
 * the dwell), so the output's .frame = j n_streams + t never decreases, as the device tracker
 * requires; with one stream that is dwell, then list order.  NaN magnitudes are outside the
 * specification.
 *
 * 32-bit arithmetic on the device: out_unit's limit gives v_max < 2^31, so every |v_m| fits an
 * int32; floor((2 v + p) / (2 p)) is computed as floor(v / p) plus one if twice the remainder
 * reaches p, which stays within int32; .doppler is formed from the uint32 v + v_max < 2^32 in the
 * same way.  A record lies in at most ceil(K / step) dwells, and max_recs ceil(K / step) < 2^31
 * bounds every (dwell, record) index. */
typedef struct fmcw_vplot {   /* 32 bytes: fmcw_tws_dev_enqueue takes it at stride 32 */
  uint32_t frame;            /* j n_streams + t: dwell j of stream t */
  uint16_t range;            /* P's */
  uint16_t doppler;          /* floor((2 (v + v_max) + out_unit) / (2 out_unit)): the unfolded axis */
  float mag;                 /* P's, bit for bit */
  int32_t v_fine;            /* v of the best hypothesis, in fine units (f0 / n_doppler) */
  int16_t fold;              /* its m */
  uint8_t n_hits;            /* positions of the dwell that hold the target, P's included */
  uint8_t hit_mask;          /* bit i' set for a hit at position i' */
  float sum_mag;             /* fp32 sum of the hit records' mag in ascending position */
  uint16_t pos;              /* P's position i in the dwell */
  uint16_t n_ties;           /* hypotheses with n_hits hits, the best included */
  uint32_t src;              /* index of P in the input list (its plot centroid is there) */
} fmcw_vplot;
typedef struct fmcw_unfold_config {   /* 23 words, 92 bytes */
  uint32_t n_range;          /* 1..65536 */
  uint32_t n_doppler;        /* 2 tol_doppler + 1 .. 65536 */
  uint32_t n_prf;            /* K, 2..8 */
  uint32_t prf_units[8];     /* p_k, 1..4096, pairwise distinct over the first K; the rest is ignored */
  uint32_t prf_phase;        /* 0..K-1 */
  uint32_t step;             /* 1..K: scans from one dwell to the next */
  uint32_t zero_bin;         /* 0..n_doppler-1: the bin of zero Doppler (0, or n_doppler / 2 for shifted bins) */
  uint32_t v_max;            /* fine units, 0 .. 32 n_doppler min p_k */
  uint32_t out_unit;         /* 1..65535 fine units per output Doppler bin, 2 v_max / out_unit + 1 <= 65535 */
  uint32_t tol_range;        /* 0..4 */
  uint32_t tol_doppler;      /* 0..4 */
  uint32_t m_of;             /* 1..K: hits a report needs */
  uint32_t n_streams;        /* 1..4096 */
  uint32_t max_recs;         /* most records one call examines, >= 1, max_recs ceil(K / step) < 2^31;
                                scratch per (dwell, record) pair, at most ceil(K / step) per record:
                                4 B + 1 bit, and 8 B per 1024 of them */
  uint32_t max_frames;       /* most frames (scans * n_streams) one call covers: >= n_streams, a multiple
                                of it, max_frames K < 2^31; scratch: 4 (K + 1) B per frame */
  int32_t device_id;         /* 0..63 */
} fmcw_unfold_config;
typedef struct fmcw_unfolder fmcw_unfolder;
/* Status words of fmcw_unfold_enqueue (status_dev). */
#define FMCW_UNFOLD_STATUS_WORDS 4
/* Defaults: 1024 x 128, K 3 with units 8 / 9 / 10, phase 0, step 3, zero_bin 0, v_max 2 * 128 * 8,
 * out_unit 8, tolerances 1 / 1, m_of 2, 1 stream, max_recs 2^20, max_frames 1024, device 0. */
void fmcw_unfold_config_default(fmcw_unfold_config* cfg);
/* Validates every field before any device access (FMCW_EINVAL, the message names the field), then
 * FMCW_ENODEV / FMCW_ENOMEM as fmcw_plots_create.  Allocates all scratch. */
int fmcw_unfold_create(const fmcw_unfold_config* cfg, fmcw_unfolder** out);
int fmcw_unfold_destroy(fmcw_unfolder* u);   /* NULL is FMCW_OK */
/* Device pointers only; stream-ordered, allocates nothing, never synchronises, uses no atomic and
 * keeps no state between calls: every word a later launch reads is written by an earlier launch of
 * the same call, so it can be captured into a hipGraph (after fmcw_plots_enqueue or
 * fmcw_merge_enqueue, before fmcw_tws_dev_enqueue) and replayed.  One stream at a time per
 * unfolder.  rec_stride is 16 or 32; recs_dev and out_dev are 16-byte aligned; n_scans * n_streams
 * <= max_frames (FMCW_EINVAL otherwise, before any device access).  Examines n = min(n_recs_dev[0],
 * rec_cap, max_recs) records (n is read on the device) and writes FMCW_UNFOLD_STATUS_WORDS words:
 *   status_dev[0] reports found (may exceed out_cap: then the first out_cap are written and nothing
 *                 is stored beyond them),
 *   status_dev[1] n_recs_dev[0] - n, the records not examined,
 *   status_dev[2] the examined records whose frame >= n_scans * n_streams.  They form a suffix and
 *                 are ignored: never a hit, never a report, and no memory is indexed by them,
 *   status_dev[3] reports found whose n_ties > 1.
 * With n = 0 it writes {0, n_recs_dev[0], 0, 0} and touches nothing else. */
int fmcw_unfold_enqueue(fmcw_unfolder* u, const void* recs_dev, size_t rec_stride, size_t rec_cap,
                        const uint32_t* n_recs_dev, size_t n_scans, fmcw_vplot* out_dev, size_t out_cap,
                        uint32_t* status_dev, void* stream);
/* Test hook: bounds the workgroups of the unfolder's tile kernels (index, find, emit), which stride
 * over 1024-item tiles.  0 = the built-in bound (4096), else min(that bound, grid).  Reports never
 * depend on it. */
int fmcw_unfold_set_grid_for_test(fmcw_unfolder* u, uint32_t grid);

/* ---- Bearing estimation: rx snapshots and angle per detection ---------------------------
 * With n_rx > 1 the path integrates the channels non-coherently (FMCW_MAG_ABS) and the phase
 * across them, which carries a target's angle, is gone from every output of fmcw_enqueue.  The
 * estimator recomputes, for each record of a detection or plot list, the one Doppler bin of the
 * one range row per channel from the corner-turned spectrum of fmcw_range_ct (spec
 * [frame][rx][range][chirp], complex fp32, range window applied, scaled by 2^-range_shift, no
 * Doppler window) and compares the channels' phases.  It is an object of its own, not part of
 * fmcw_handle / fmcw_config; the reference (one receive channel) has no such stage.
 *
 * Input: a record list and its count word.  A record is any element that begins with
 * {uint32 frame; uint16 range; uint16 doppler}: fmcw_det (stride 16) or fmcw_plot (stride 32).
 * Order is free and duplicates are allowed.
 *
 * Snapshot of record i = (f, r, d), channel k = 0 .. n_rx - 1:
 *   s_k = sum_c w[c] y_k[c] exp(-2 pi i d c / n_doppler),   c = 0 .. n_doppler - 1,
 * y_k the canceller of mti_mode over x_k[c] = spec[f][k][r][c] (OFF: x[c]; 2-pulse: x[c] - x[c-1];
 * 3-pulse: x[c] - 2 x[c-1] + x[c-2]; the delay line is zero before chirp 0), and w the library's
 * fp32 Hamming table of n_doppler points (the values fmcw_enqueue multiplies by), or all ones for
 * FMCW_WIN_NONE.  The float paths only: no Q15 window, no compat MTI.  With the handle's own window
 * and mti_mode, s_k is the complex value whose magnitude the map holds.
 *
 * Bearing, for a uniform line array with element k at k * spacing wavelengths:
 *   P = sum_{k=0}^{n_rx-2} s_{k+1} conj(s_k)
 *   nu = arg(P) / (2 pi)        cycles per element, in [-0.5, 0.5] (atan2's +0.5 on the branch cut)
 *   sin_theta = nu / spacing
 *   power = sqrt(sum_k |s_k|^2)                  the NCI magnitude of the cell
 *   coherence = |P| / sum_{k=0}^{n_rx-2} |s_{k+1}| |s_k|   1 for one plane wave, lower when two
 *                                targets share the cell; 0 if the denominator is 0 or not finite
 * The closed-form phase comparison, not a scan over an angle grid: O(n_rx), and no argmax to differ
 * between precisions.  Callers who want more (MUSIC, a Bartlett scan) take the snapshots; the scan
 * over a steering table with successive cancellation is fmcw_doa_* below. */
#define FMCW_BEARING_NO_ANGLE 1u      /* |sin_theta| > 1: no real angle */
#define FMCW_BEARING_ONE_RX 2u        /* n_rx == 1: nu = 0, sin_theta = 0, coherence = 0 */
#define FMCW_BEARING_OUT_OF_RANGE 4u  /* frame >= n_frames of the call, range >= n_range or doppler >=
                                         n_doppler: no memory is read, every other field of the
                                         output record (and its snapshot) is zero */
typedef struct fmcw_bearing {   /* 32 bytes */
  uint32_t frame;              /* the record's cell, copied (zero with FMCW_BEARING_OUT_OF_RANGE) */
  uint16_t range;
  uint16_t doppler;
  uint32_t flags;              /* FMCW_BEARING_* bits */
  float nu;
  float sin_theta;
  float power;
  float coherence;
  uint32_t reserved;           /* written as 0 */
} fmcw_bearing;
typedef struct fmcw_bearings_config {   /* 32 bytes */
  uint32_t n_range;            /* as fmcw_config: power of two, 64..8192 */
  uint32_t n_doppler;          /* as fmcw_config: power of two, 32..1024 */
  uint32_t n_rx;               /* 1..64 */
  int32_t window;              /* FMCW_WIN_NONE or FMCW_WIN_HAMMING */
  int32_t mti_mode;            /* fmcw_mti_mode */
  float spacing;               /* element spacing in wavelengths, > 0 and finite */
  uint32_t max_records;        /* most records one call processes, 1..2^31-1 (no scratch depends on it) */
                               /* device memory of an estimator: 12 B per Doppler bin + 8 KiB */
  int32_t device_id;           /* 0..63 */
} fmcw_bearings_config;
typedef struct fmcw_bearings fmcw_bearings;
/* Status words of fmcw_bearings_enqueue (n_out_dev). */
#define FMCW_BEARING_STATUS_WORDS 2
/* Defaults: 1024, 128, 1 rx, Hamming, MTI off, spacing 0.5, max_records 2^20, device 0. */
void fmcw_bearings_config_default(fmcw_bearings_config* cfg);
/* Validates before any device access (FMCW_EINVAL, the message names the field), then
 * FMCW_ENODEV / FMCW_ENOMEM as fmcw_create.  Uploads the twiddle and window tables (n_doppler
 * entries each, computed in fp64). */
int fmcw_bearings_create(const fmcw_bearings_config* cfg, fmcw_bearings** out);
int fmcw_bearings_destroy(fmcw_bearings* b);   /* NULL is FMCW_OK */
/* Device pointers only; stream-ordered, allocates nothing, never synchronises and keeps no state
 * between calls, so it can be captured into a hipGraph after fmcw_range_ct and fmcw_enqueue on the
 * same stream and replayed.  One stream at a time per estimator (its 8 KiB of per-workgroup
 * counts are shared by its calls).
 * spec_dev: n_frames frames as fmcw_range_ct writes them for (n_range, n_doppler, n_rx).
 * records_dev: rec_cap records of rec_stride bytes (16 or 32, else FMCW_EINVAL), 4-byte aligned.
 * Processes n = min(n_records_dev[0], rec_cap, max_records) records (n is read on the device):
 *   bearings_dev[i], i < n (16-byte aligned, room for min(rec_cap, max_records) records); nothing
 *                  is stored beyond them,
 *   snaps_dev[i * n_rx + k] = s_k as complex fp32 (8-byte aligned), unless snaps_dev is NULL,
 *   n_out_dev[0] = n, n_out_dev[1] = the out-of-range records among them.
 * With n = 0 it writes {0, 0} and touches nothing else. */
int fmcw_bearings_enqueue(fmcw_bearings* b, const void* spec_dev, size_t n_frames,
                          const void* records_dev, size_t rec_stride, size_t rec_cap,
                          const uint32_t* n_records_dev, fmcw_bearing* bearings_dev, void* snaps_dev,
                          uint32_t* n_out_dev, void* stream);
/* Test hook: bounds the workgroups of the estimator's kernel, whose waves stride over the records,
 * so that a short list drives a workgroup through several records.  0 = the built-in bound (2048),
 * else min(that bound, grid).  Results never depend on it. */
int fmcw_bearings_set_grid_for_test(fmcw_bearings* b, uint32_t grid);

/* ---- Coherent beamforming: per-beam range-Doppler maps from the rx channels --------------
 * With n_rx > 1 fmcw_enqueue sums the channels' powers (FMCW_MAG_ABS: sqrt(sum_rx |X_rx|^2)), which
 * gains about sqrt(n_rx) in SNR.  The beamformer applies a complex weight matrix to the channels of
 * fmcw_range_ct's spectrum BEFORE the Doppler transform, so a beam steered at a target gains n_rx,
 * and two targets that share a range-Doppler cell separate in angle.  Its maps go to fmcw_cfar as
 * any caller-supplied map does.  An object of its own, not part of fmcw_handle / fmcw_config; the
 * reference (one receive channel) has no such stage.
 *
 * For frame f, beam b, range row r:
 *   y_b[c] = sum_{k=0}^{n_rx-1} W[b][k] x_k[c],   x_k[c] = spec[f][k][r][c]
 * (spec as fmcw_range_ct writes it: complex fp32, range window applied, no Doppler window),
 *   z_b = the canceller of mti_mode over y_b, as the bearing estimator defines it (OFF: y[c];
 *         2-pulse: y[c] - y[c-1]; 3-pulse: y[c] - 2 y[c-1] + y[c-2]; zero delay line before chirp 0),
 *   maps[f][b][r][d] = | sum_c w[c] z_b[c] exp(-2 pi i d c / n_doppler) |,
 * w the library's fp32 Hamming table of n_doppler points (the values fmcw_enqueue multiplies by), or
 * all ones for FMCW_WIN_NONE.  The float paths only: no Q15 window, no compat MTI, no AMBM, no dB map.
 * Window and canceller are linear per chirp: the kernel may apply them per channel or per beam; this
 * header defines the result, not the order.  The channels are summed in the order k = 0 .. n_rx - 1,
 * so a map's bytes depend on spec and W alone.
 *
 * Weights: weights_host holds n_beams x n_rx complex fp32 values, interleaved re, im, row-major
 * [beam][rx], copied to the device at create (no update afterwards); every component must be finite.
 * Steering, taper and channel calibration are the caller's: the library applies the matrix and
 * nothing else.  With n_rx == 1 and W = [[1]] the map is fmcw_enqueue's single-channel linear map
 * for the same window and mti_mode.
 *
 * Layout: maps_dev is [frame][beam][range][doppler] float32, 16-byte aligned.  Each (frame, beam)
 * map is contiguous, so fmcw_cfar(h, maps_dev, n_frames * n_beams, ...) runs on it unchanged with a
 * handle whose max_frames >= n_frames * n_beams; a detection's .frame is then f * n_beams + b. */
typedef struct fmcw_beams_config {   /* 32 bytes */
  uint32_t n_range;            /* as fmcw_config: power of two, 64..8192 */
  uint32_t n_doppler;          /* as fmcw_config: power of two, 32..1024 */
  uint32_t n_rx;               /* 1..64 */
  uint32_t n_beams;            /* 1..64 */
  int32_t window;              /* FMCW_WIN_NONE or FMCW_WIN_HAMMING (Doppler window) */
  int32_t mti_mode;            /* fmcw_mti_mode */
  uint32_t reserved;           /* must be 0 */
                               /* device memory of a beamformer: the weight matrix (8 B x n_beams x
                                  n_rx) and the window table (4 B per Doppler bin), nothing else */
  int32_t device_id;           /* 0..63 */
} fmcw_beams_config;
typedef struct fmcw_beams fmcw_beams;
/* Defaults: 1024, 128, 1 rx, 1 beam, Hamming, MTI off, device 0. */
void fmcw_beams_config_default(fmcw_beams_config* cfg);
/* Validates cfg and weights_host before any device access (FMCW_EINVAL, the message names the
 * field), then FMCW_ENODEV / FMCW_ENOMEM as fmcw_bearings_create.  Uploads the weights and the
 * window table. */
int fmcw_beams_create(const fmcw_beams_config* cfg, const float* weights_host, fmcw_beams** out);
int fmcw_beams_destroy(fmcw_beams* b);   /* NULL is FMCW_OK */
/* Device pointers only; stream-ordered, allocates nothing, never synchronises and keeps no state
 * between calls (it has no scratch), so it can be captured into a hipGraph after fmcw_range_ct on
 * the same stream and replayed.  One stream at a time per beamformer.
 * spec_dev: n_frames frames as fmcw_range_ct writes them for (n_range, n_doppler, n_rx).
 * maps_dev: n_frames * n_beams maps (above); nothing is stored beyond them.
 * n_frames == 0 is FMCW_OK and launches nothing. */
int fmcw_beams_enqueue(fmcw_beams* b, const void* spec_dev, size_t n_frames, float* maps_dev,
                       void* stream);
/* Test hook: bounds the workgroups of the beamformer's persistent kernel, whose waves stride over the
 * tiles of 1024 map cells, so that a small call drives a workgroup through several tiles, frames and
 * beams.  0 = the built-in bound (the workgroups resident at once), else min(that bound, grid).
 * Results never depend on it. */
int fmcw_beams_set_grid_for_test(fmcw_beams* b, uint32_t grid);
/* Replaces the beamformer's matrix by w_dev: n_beams x n_rx complex fp32, [beam][rx] as weights_host,
 * 8-byte aligned, on the beamformer's device.  A stream-ordered device-to-device copy: capturable into
 * a hipGraph between fmcw_adapt_enqueue and fmcw_beams_enqueue on the same stream, never synchronises.
 * There is no finiteness check on the device: weights that are not finite give maps that are not
 * finite.  A beamformer that never calls this keeps the matrix of fmcw_beams_create. */
int fmcw_beams_set_weights_dev(fmcw_beams* b, const void* w_dev, void* stream);

/* ---- Adaptive beam weights (MVDR): sample covariance and loaded solve --------------------
 * The beamformer applies the matrix its caller gives it.  A strong off-axis emitter (a jammer, another
 * FMCW radar) enters a fixed beam through its sidelobes and raises the floor of every cell; the
 * detectors' thresholds rise with it.  This object chooses the weights from the data (sample matrix
 * inversion): the channels' covariance over a training window of fmcw_range_ct's spectrum, its
 * diagonal loaded, and the minimum-variance weights under a unit-gain constraint per look direction.
 * An object of its own, not part of fmcw_handle / fmcw_config; the reference has no such stage.
 *
 * Snapshots.  z_k[c] is the canceller of mti_mode over x_k[c] = spec[f][k][r][c], as the beamformer
 * defines it (OFF: x[c]; 2-pulse: x[c] - x[c-1]; 3-pulse: x[c] - 2 x[c-1] + x[c-2]; zero delay line
 * before chirp 0).  The snapshots are the vectors z = (z_0 .. z_{n_rx-1}) at all (f, r, c) with
 * f < n_frames of the call, r in [train_r0, train_r0 + train_rows) and every chirp c < n_doppler;
 * K = n_frames * train_rows * n_doppler is their count.
 *
 *   R[i][j]  = (1/K) sum z_i conj(z_j)                         sample covariance, Hermitian
 *   delta    = loading * Re tr(R) / n_rx,   Rl = R + delta I   diagonal loading
 *   W[b][k]  = conj((Rl^-1 a_b)[k]) / (a_b^H Rl^-1 a_b)        a_b = a_host[b][:], the look direction
 *
 * W is in the beamformer's convention, y = sum_k W[b][k] x_k, so sum_k W[b][k] a_b[k] = 1: a plane
 * wave with array response a_b passes beam b at unit gain, and the output power from everything else
 * is the least possible.  R = I gives W[b][k] = conj(a_b[k]) / |a_b|^2, the conventional beam
 * (fmcw.beams.steering_weights for a_b[k] = exp(2 pi i nu_b k)).
 *
 * Fallback.  Rl is factorised as L L^H (Cholesky, fp64).  If a pivot is not greater than
 * FMCW_ADAPT_PIVOT_MIN times the mean diagonal of Rl (a pivot that is zero, negative or NaN
 * included), or a beam's weights come out not finite, the call writes the conventional weights
 * conj(a_b) / |a_b|^2 (for every beam in the first case, for that beam in the second) and sets
 * FMCW_ADAPT_FALLBACK in the status words.  cov and delta are written either way.
 *
 * Precision.  The products z_i conj(z_j) are summed in fp32 on the matrix cores over units of at most
 * ceil(T / n_units) steps of 64 snapshots (T = n_frames * ceil(train_rows * n_doppler / 64),
 * n_units = min(T, 2048)), the units' partial sums and everything after them in fp64.  The partition
 * depends on the shape and n_frames alone: the bytes of W, cov and info depend on spec and the
 * configuration, never on the grid. */
#define FMCW_ADAPT_FALLBACK 1u        /* status flag: conventional weights were written */
#define FMCW_ADAPT_PIVOT_MIN 1e-8     /* least Cholesky pivot, relative to the mean diagonal of Rl */
/* Status words of fmcw_adapt_enqueue (info_dev):
 *   [0], [1]  K, low and high word
 *   [2]       flags (FMCW_ADAPT_FALLBACK)
 *   [3]       n_units, the partial sums the call formed
 *   [4], [5]  delta as the bits of an fp64, low and high word
 *   [6], [7]  written as 0 */
#define FMCW_ADAPT_INFO_WORDS 8
typedef struct fmcw_adapt_config {   /* 40 bytes */
  uint32_t n_range;            /* as fmcw_config: power of two, 64..8192 */
  uint32_t n_doppler;          /* as fmcw_config: power of two, 32..1024 */
  uint32_t n_rx;               /* 1..16 (17..64, which the beamformer takes, is not built) */
  uint32_t n_beams;            /* 1..64 */
  int32_t mti_mode;            /* fmcw_mti_mode: 0, 2 or 3 */
  uint32_t train_r0;           /* the training rows [train_r0, train_r0 + train_rows) lie in n_range */
  uint32_t train_rows;         /* >= 1 */
  float loading;               /* finite, >= 0 */
  uint32_t reserved;           /* must be 0 */
                               /* device memory of an object: the constraint matrix (8 B x n_beams x
                                  n_rx) and 2048 + 64 partial tiles (2.1 MiB for n_rx <= 8, else 8.5 MiB) */
  int32_t device_id;           /* 0..63 */
} fmcw_adapt_config;
typedef struct fmcw_adapt fmcw_adapt;
/* Defaults: 1024, 128, 1 rx, 1 beam, MTI off, training rows [0, 1024), loading 1e-2, device 0. */
void fmcw_adapt_config_default(fmcw_adapt_config* cfg);
/* a_host: n_beams x n_rx complex fp32, interleaved re, im, row-major [beam][rx]: the array response
 * of each look direction.  Every component finite and no row all zero.  Validates cfg and a_host
 * before any device access (FMCW_EINVAL, the message names the field), then FMCW_ENODEV /
 * FMCW_ENOMEM as fmcw_beams_create. */
int fmcw_adapt_create(const fmcw_adapt_config* cfg, const float* a_host, fmcw_adapt** out);
int fmcw_adapt_destroy(fmcw_adapt* a);   /* NULL is FMCW_OK */
/* Device pointers only; stream-ordered, allocates nothing and never synchronises.  Every scratch word
 * it reads is written earlier in the same call and nothing is zeroed between calls, so it can be
 * captured into a hipGraph after fmcw_range_ct on the same stream and replayed.  One stream at a time
 * per object.
 * spec_dev: n_frames frames as fmcw_range_ct writes them for (n_range, n_doppler, n_rx), 8-byte aligned.
 * w_dev:    W, n_beams x n_rx complex fp32 [beam][rx], 8-byte aligned: fmcw_beams_set_weights_dev's input.
 * cov_dev:  R, n_rx x n_rx complex fp64 row-major, 16-byte aligned; NULL: not written.
 * info_dev: FMCW_ADAPT_INFO_WORDS words (above).
 * Nothing is stored beyond them.  n_frames == 0 is FMCW_OK and launches nothing. */
int fmcw_adapt_enqueue(fmcw_adapt* a, const void* spec_dev, size_t n_frames, void* w_dev, void* cov_dev,
                       uint32_t* info_dev, void* stream);
/* Test hook: bounds the workgroups of the accumulation kernel, whose waves stride over the units, so
 * that a small call drives a wave through several units.  0 = the built-in bound (512), else
 * min(that bound, grid).  Results never depend on it. */
int fmcw_adapt_set_grid_for_test(fmcw_adapt* a, uint32_t grid);

/* ---- Cell-averaging CFAR (CA / GO / SO): a detector whose cost does not depend on the data ----
 * The reference's detectors are the two ordered-statistic CFARs; this is the cell-averaging family
 * beside them, an object of its own (not part of fmcw_handle / fmcw_config).  It does the same
 * arithmetic on every cell whatever the map holds, so a caller can budget it, for instance under the
 * beamformer's n_frames * n_beams maps.  It is not a replacement for OS-CFAR on heavy-tailed clutter.
 * Everything below is fp32.
 *
 * Input.  map[f][r][d] float32, [frame][range][doppler], as fmcw_enqueue and fmcw_beams_enqueue write
 * it.  Cells enter as fmcw_cfar takes them: negative cells and -0.0 become +0.  NaN is outside the
 * specification.  +Inf follows IEEE arithmetic as written.
 *
 * Window.  ref_range (Rr), guard_range (Gr), ref_doppler (Rd), guard_doppler (Gd), each named by the
 * axis it acts on, as the cfar2d_* fields are.  Half extents Hr = Rr + Gr, Hd = Rd + Gd.  Doppler is
 * circular.  A CUT is tested only when Hr <= r < n_range - Hr; elsewhere there is no detection (the
 * build's rule for the 2-D OS-CFAR).  Reference set: the (2Hr+1) x (2Hd+1) window minus
 * the (2Gr+1) x (2Gd+1) guard block; N = (2Hr+1)(2Hd+1) - (2Gr+1)(2Gd+1), 128 with the defaults
 * 4/1/4/2.
 *
 * Canonical sums.  These shared partial sums are the definition: a kernel that computes each once per
 * cell and shares it between the CUTs that use it is bit-exact by construction.  A sum "in ascending
 * order" starts from its first term and adds the next terms one at a time; an empty sum is +0.0.
 * Row-wise, Doppler indices mod n_doppler:
 *   Lg[r][d] = sum of m[r][d+dd] for dd = -Hd .. -Gd-1, in ascending order,
 *   Cg[r][d] = the same for dd = -Gd .. Gd,
 *   Rg[r][d] = the same for dd = Gd+1 .. Hd,
 *   H[r][d]  = (Lg + Cg) + Rg.
 * Column-wise, in ascending dr:
 *   U = sum of H[r+dr][d]  for dr = -Hr .. -Gr-1,     D = the same for dr = Gr+1 .. Hr,
 *   L = sum of Lg[r+dr][d] for dr = -Gr .. Gr,        R = sum of Rg[r+dr][d] for dr = -Gr .. Gr.
 * Halves: A = U + L (rows above, left segments), B = D + R (rows below, right segments); N/2 cells
 * each.
 *
 * Threshold, one multiplication:  CA: T = kc * (A + B), kc = (float)((double)alpha / N);
 * GO: T = kh * max(A, B);  SO: T = kh * min(A, B), kh = (float)((double)alpha / (N/2)).  The
 * constants are formed once on the host.  There is no division and no multiply-add anywhere, so no
 * contraction can change a bit.
 *
 * Decision and order.  Detect iff m_cut > T (strict).  The record is {frame, range, doppler,
 * mag = m_cut, threshold = T}.  The list is strictly increasing in (frame, range, doppler), which is
 * what the plot extractor requires of its input.
 *
 * Degenerate windows are allowed and fall out of the same formulas: Rr = 0 is a 1-D CA along Doppler
 * (U = D = 0), Rd = 0 a 1-D CA along range.
 *
 * Validation: each ref in 0..8, each guard in 0..4, N >= 2, 2Hd + 1 <= n_doppler, 2Hr + 1 <= n_range. */
typedef enum { FMCW_CACFAR_CA = 0, FMCW_CACFAR_GO = 1, FMCW_CACFAR_SO = 2 } fmcw_cacfar_mode;
typedef struct fmcw_cacfar_config {   /* 12 words, 48 bytes */
  uint32_t n_range;            /* as fmcw_config: power of two, 64..8192 */
  uint32_t n_doppler;          /* as fmcw_config: power of two, 32..1024 */
  int32_t mode;                /* fmcw_cacfar_mode */
  uint32_t ref_range;          /* Rr, 0..8 */
  uint32_t guard_range;        /* Gr, 0..4 */
  uint32_t ref_doppler;        /* Rd, 0..8 */
  uint32_t guard_doppler;      /* Gd, 0..4 */
  float alpha;                 /* finite, > 0 */
  uint32_t max_frames;         /* >= 1; max_frames x n_range x n_doppler < 2^32 */
                               /* device memory of a detector: 8 B per tile of max_frames (a tile is
                                  max(64, 65536 / n_doppler) range rows of a frame, or the whole frame
                                  when n_range is smaller): a count and an offset.  No per-cell
                                  scratch, so well under 1 bit per cell */
  int32_t device_id;           /* 0..63 */
  uint32_t reserved[2];        /* must be 0 */
} fmcw_cacfar_config;
typedef struct fmcw_cacfar fmcw_cacfar;
/* Defaults: 1024, 128, CA, window 4/1/4/2, alpha 4.0, max_frames 1, device 0. */
void fmcw_cacfar_config_default(fmcw_cacfar_config* cfg);
/* Validates every field before any device access (FMCW_EINVAL, the message names the field, *out is
 * NULL), then FMCW_ENODEV / FMCW_ENOMEM as fmcw_beams_create. */
int fmcw_cacfar_create(const fmcw_cacfar_config* cfg, fmcw_cacfar** out);
int fmcw_cacfar_destroy(fmcw_cacfar* c);   /* NULL is FMCW_OK */
/* Device pointers only; stream-ordered, allocates nothing, never synchronises and keeps no state
 * between calls, so it can be captured into a hipGraph after fmcw_enqueue or fmcw_beams_enqueue on the
 * same stream and replayed.  One stream at a time per detector (its per-tile words are shared by its
 * calls).  Three launches: a count pass (per-tile counts, tiles in (frame, range) order), a scan of
 * the counts, and an emit pass that recomputes and stores at the scanned offsets: two reads of the
 * map, whatever it holds.
 * map_dev: n_frames maps, 16-byte aligned; n_frames > max_frames is FMCW_EINVAL.
 * n_dets_dev: FMCW_STATUS_WORDS words: [0] the detections found (may exceed det_cap: then the first
 *   det_cap records of the ordered list are written and nothing is stored beyond them), [1..3] 0; so
 *   fmcw_gather_dets, the plot extractor and the bearing estimator take the list and the words
 *   unchanged.  The list is complete and ordered at any density.
 * dets_dev: det_cap records, 16-byte aligned; may be NULL with det_cap = 0, which counts only.
 * n_frames == 0 writes four zero words and touches no record. */
int fmcw_cacfar_enqueue(fmcw_cacfar* c, const float* map_dev, size_t n_frames, fmcw_det* dets_dev,
                        size_t det_cap, uint32_t* n_dets_dev, void* stream);
/* Test hook: bounds the workgroups of the two persistent passes, which stride over the tiles, so that
 * a small call drives a workgroup through several tiles and frames.  0 = the built-in bound (the
 * workgroups resident at once), else min(that bound, grid).  Results never depend on it. */
int fmcw_cacfar_set_grid_for_test(fmcw_cacfar* c, uint32_t grid);

/* ---- Clutter map (Nitzberg's clutter-map CFAR): a threshold per cell from the cell's own history ----
 * Every detector above estimates its threshold from a cell's spatial neighbours within one frame, which
 * goes wrong at a clutter edge (the window straddles two levels) and in range-dependent clutter.  The
 * clutter map looks at the same cell in earlier scans instead: a per-cell exponential average over scans,
 * and a cell is detected when it exceeds a multiple of its own history.  An object of its own (not part
 * of fmcw_handle / fmcw_config), and the first stage whose state is a function of the maps and lives on
 * the device between calls.  Everything below is fp32, and every operation is rounded on its own: there
 * is no multiply-add, so no contraction can change a bit.
 *
 * Streams.  n_streams (B) independent maps, one per beam or sensor.  Frame f of a call belongs to stream
 * f % B, the order in which fmcw_beams_enqueue writes its n_frames * n_beams maps; a call's n_frames is
 * a multiple of B, and its n_frames / B scans of a stream are taken in frame order.
 *
 * State, device memory owned by the object, persistent between calls.  Per stream a plane c[r][d] of
 * float32 and an age word (uint32, the scans taken since the last reset, saturating at 0xFFFFFFFF).
 * Create and fmcw_cmap_reset set every age to 0; the planes' contents are then irrelevant.
 *
 * One scan of stream b, map m, age a.  Per cell (r, d):
 *   x = m > 0 ? m : +0        negative cells and -0.0 become +0, as for fmcw_cfar and the
 *                             cell-averaging detector; NaN and Inf are outside the specification.
 *   a == 0:  c' = x, and no cell is tested.
 *   a >= 1:  every term uses the state from before this scan's update:
 *     M  = the maximum of c[r+dr][(d+dd) mod n_doppler] over dr = -Sr .. Sr, dd = -Sd .. Sd
 *          (spread_range Sr, spread_doppler Sd), rows 0 <= r+dr < n_range only: range is clipped, Doppler
 *          is circular.  A maximum is exact in any order.
 *     T  = fmaxf(alpha * M, floor)
 *     detect iff a >= warmup and x > T (strict); the record is {frame, range, doppler, mag = x,
 *          threshold = T}, frame being the frame's index within the call.
 *     u  = x when clip == 0, else fminf(x, fmaxf(clip * c, floor)), c being the cell's own value: this
 *          limits how fast a target burns into the map.
 *     t  = u - c;  p = gain * t;  c' = c + p      three operations, three roundings.
 *   After the scan: a' = min(a + 1, 0xFFFFFFFF).
 * The update is unconditional: it does not depend on the decision.  A cell's recurrence then depends only
 * on the cell's own history (x and c), never on a neighbour's, so a workgroup can recompute the
 * recurrence of the halo rows it needs for M without exchanging anything with its neighbours, and the
 * state does not depend on det_cap.  A persistent target therefore raises its own threshold; clip bounds
 * the rate.
 *
 * Order.  The list is strictly increasing in (frame, range, doppler), which is what the plot extractor
 * requires of its input.  Every row is tested: there is no excluded border.
 *
 * Planes given to fmcw_cmap_set_state hold finite values >= +0 (what a scan leaves behind); anything else
 * is outside the specification. */
typedef struct fmcw_cmap_config {   /* 16 words, 64 bytes */
  uint32_t n_range;            /* as fmcw_config: power of two, 64..8192 */
  uint32_t n_doppler;          /* as fmcw_config: power of two, 32..1024 */
  uint32_t n_streams;          /* B, 1..64 */
  float gain;                  /* g: finite, 0 < g <= 1 */
  float alpha;                 /* finite, > 0 */
  float floor;                 /* finite, >= 0: the least threshold, and the least clip level */
  float clip;                  /* 0 (off), or finite and >= 1 */
  uint32_t spread_range;       /* Sr, 0..4 */
  uint32_t spread_doppler;     /* Sd, 0..4; 2 Sd + 1 <= n_doppler */
  uint32_t warmup;             /* >= 1: no detection while a stream's age is below it */
  uint32_t max_frames;         /* a multiple of B, >= B; max_frames x n_range x n_doppler < 2^32 */
                               /* device memory of a map: two copies of the B planes (a call reads one
                                  and writes the other, so that a workgroup never reads a halo row its
                                  neighbour has already written), 8 B per tile of max_frames (a tile is
                                  8192 / n_doppler range rows of a frame, or the whole frame when
                                  n_range is smaller), and 8 B per stream */
  int32_t device_id;           /* 0..63 */
  uint32_t reserved[4];        /* must be 0 */
} fmcw_cmap_config;
typedef struct fmcw_cmap fmcw_cmap;
/* Defaults: 1024, 128, 1 stream, gain 0.125, alpha 4.0, floor 0, clip 0, spread 1/1, warmup 8,
 * max_frames 1, device 0. */
void fmcw_cmap_config_default(fmcw_cmap_config* cfg);
/* Validates every field before any device access (FMCW_EINVAL, the message names the field, *out is
 * NULL), then FMCW_ENODEV / FMCW_ENOMEM as fmcw_cacfar_create.  Every age starts at 0. */
int fmcw_cmap_create(const fmcw_cmap_config* cfg, fmcw_cmap** out);
int fmcw_cmap_destroy(fmcw_cmap* c);   /* NULL is FMCW_OK */
/* Device pointers only; stream-ordered, allocates nothing and never synchronises; the ages are read on
 * the device, never on the host.  It can therefore be captured into a hipGraph after fmcw_enqueue or
 * fmcw_beams_enqueue on the same stream; the state advances by the call's scans at every replay.  One
 * stream at a time per map.  Three launches whatever n_frames is: a count pass over (stream, tile) units
 * that runs all of the call's scans for its tile and leaves the state alone, a scan of the per-(frame,
 * tile) counts, and an emit pass that repeats the arithmetic, stores the records and writes the state.
 * map_dev: n_frames maps, 16-byte aligned; n_frames > max_frames, or not a multiple of n_streams, is
 *   FMCW_EINVAL.
 * n_dets_dev: FMCW_STATUS_WORDS words: [0] the detections found (may exceed det_cap: then the first
 *   det_cap records of the ordered list are written and nothing is stored beyond them), [1..3] 0.
 * dets_dev: det_cap records, 16-byte aligned; may be NULL with det_cap = 0.  The state advances by the
 *   call's scans whatever det_cap is.
 * n_frames == 0 writes four zero words and leaves the state alone. */
int fmcw_cmap_enqueue(fmcw_cmap* c, const float* map_dev, size_t n_frames, fmcw_det* dets_dev, size_t det_cap,
                      uint32_t* n_dets_dev, void* stream);
/* Every age goes to 0, in stream order. */
int fmcw_cmap_reset(fmcw_cmap* c, void* stream);
/* Stream-ordered copies of the state, for checkpoints and tests: planes_dev holds n_streams planes
 * [stream][range][doppler] (16-byte aligned), ages_dev n_streams words (4-byte aligned).
 * fmcw_cmap_get_state: either pointer may be NULL (that part is not copied), not both.
 * fmcw_cmap_set_state: planes_dev is required; ages_dev may be NULL, which keeps the ages.  A NULL
 * planes_dev is FMCW_EINVAL: ages without the planes they describe would make the next scan test against
 * whatever the planes held. */
int fmcw_cmap_get_state(fmcw_cmap* c, float* planes_dev, uint32_t* ages_dev, void* stream);
int fmcw_cmap_set_state(fmcw_cmap* c, const float* planes_dev, const uint32_t* ages_dev, void* stream);
/* Test hook: bounds the workgroups of the two persistent passes, which stride over the (stream, tile)
 * units.  0 = the built-in bound (the workgroups resident at once), else min(that bound, grid).  Results
 * never depend on it. */
int fmcw_cmap_set_grid_for_test(fmcw_cmap* c, uint32_t grid);

/* ---- Track-while-scan tracker (host side) ----------------------------------------------
 * Replaces rtl/src/tws_tracker.vhd (radar_core.vhd:424-438): MAX_TRACKS alpha-beta tracks in
 * Q2 bins with Q8 gains over the detection list, one scan (= one frame's detections) per
 * fmcw_tws_scan.  CPU code: serial, <= 64 detections x 64 tracks per scan.  The same tracker over a
 * device-resident list, many scans and independent track files per call, is fmcw_tws_dev_* below.
 * rtl_compat = 1 is the VHDL bit for bit (wrapping field widths, the signal read of
 * best_distance in ASSOCIATE, the 6-bit detection counter); 0 is the intended tracker (wide
 * integers, nearest-neighbour association).  Output: firm and coasting tracks in track-file
 * order, as ST_OUTPUT streams them (:273-295); *n_out = their count (FMCW_EDETCAP if > cap). */
typedef struct fmcw_tws fmcw_tws;
typedef struct {
  uint32_t max_tracks;   /* MAX_TRACKS (32), <= 64 */
  uint32_t max_dets;     /* detections kept per scan (64, the RTL's MAX_DETS), <= 64 */
  uint32_t init_hits;    /* INIT_HITS (2) */
  uint32_t coast_max;    /* COAST_MAX (5) */
  uint32_t gate_r;       /* ASSOC_GATE_R (10 range bins) */
  uint32_t gate_d;       /* ASSOC_GATE_D (5 Doppler bins) */
  uint32_t alpha_q8;     /* ALPHA_GAIN (128 = 0.5), < 256 */
  uint32_t beta_q8;      /* BETA_GAIN (64 = 0.25), < 256 */
  int32_t rtl_compat;
} fmcw_tws_config;
typedef struct {
  uint16_t id;           /* trk_id: track-file slot */
  uint8_t status;        /* trk_status: 2 FIRM, 3 COAST */
  uint8_t quality;       /* trk_quality 0..15 */
  int32_t range_q2;      /* trk_range: range bin x 4 */
  int32_t doppler_q2;    /* trk_doppler: Doppler bin x 4 */
  int32_t vel_r;         /* trk_vel_r: Q2 range bins per scan */
  int32_t vel_d;         /* trk_vel_d */
  uint32_t last_mag;     /* last associated detection magnitude (rounded) */
  uint32_t age;          /* scans since initiation */
} fmcw_track;
void fmcw_tws_config_default(fmcw_tws_config* cfg);
int fmcw_tws_create(const fmcw_tws_config* cfg, fmcw_tws** out);
int fmcw_tws_destroy(fmcw_tws* t);
int fmcw_tws_scan(fmcw_tws* t, const fmcw_det* dets, size_t n_dets, fmcw_track* out, size_t cap,
                  size_t* n_out, uint32_t* n_active);

/* ---- Track-while-scan tracker (device side) --------------------------------------------
 * fmcw_tws_scan on the GPU, over a record list that is already there: the list and count word that
 * fmcw_enqueue, fmcw_cfar, fmcw_cacfar_enqueue or fmcw_plots_enqueue wrote go in as they are, so a
 * caller who wants tracks no longer synchronises, copies the list back and slices it by frame, and
 * the whole chain can be captured into one hipGraph.  An object of its own, not part of fmcw_handle.
 * The host tracker above stays the default and is the second reference of this one's tests.
 *
 * Records begin with {uint32 frame; uint16 range; uint16 doppler; float mag}: rec_stride is 16
 * (fmcw_det) or 32 (fmcw_plot).  .frame must be non-decreasing along the list (those four producers
 * guarantee it).  The kernels examine n = min(n_recs_dev[0], rec_cap) records; n is read on the device.
 *
 * Scans and streams.  A tracker holds n_streams independent track files.  Record frame m belongs to
 * scan m / n_streams of stream m % n_streams, which is the beamformer's frame = f * n_beams + b; with
 * n_streams = 1 a frame is a scan.  A call runs scans 0 .. n_scans-1 of every stream in order; a
 * (scan, stream) without records is still a scan (its tracks coast), as fmcw_tws_scan with n_dets = 0.
 *
 * Per scan: the detections are the scan's records in list order (the first max_dets are kept), and
 * everything else is fmcw_tws_scan statement for statement for both rtl_compat values: the magnitude
 * rounding (<= 0 gives 0, >= 4e9 all ones, else (uint64)(m + 0.5f); a NaN magnitude is outside the
 * specification), the RTL's wrapping widths, RESIZE and 6-bit detection counter, the best_distance /
 * best_idx signal carried from one active track to the next, from scan to scan and from call to call
 * (kept per stream, with the power-up value), nearest-neighbour association with the lowest index
 * winning ties in the intended mode, INITIATE in detection order into the lowest free slot.  Integers
 * are 64-bit on the device as on the host.
 *
 * State is device-resident and persists between calls: two calls of 8 scans equal one call of 16.  A
 * captured graph that is replayed therefore ADVANCES the track files on every replay (a replay is
 * another n_scans scans, not a repetition of the same ones); fmcw_tws_dev_reset, itself capturable,
 * puts every track file back to power-up.  One stream at a time per tracker.
 *
 * Output, fixed stride, no compaction.  With m = scan * n_streams + stream:
 *   tracks_dev[m * track_cap + j], j < min(n_out, track_cap): the firm and coasting tracks in
 *     track-file order (the records fmcw_tws_scan returns for that scan); slots beyond are untouched;
 *   counts_dev[2 m] = n_out (may exceed track_cap), counts_dev[2 m + 1] = n_active.
 *   status_dev[0] = n_recs_dev[0] - n, the records not examined;
 *   status_dev[1] = examined records whose frame is >= n_scans * n_streams: ignored, and no memory is
 *     indexed by them.
 * The last kernel of every call that returns FMCW_OK writes the status words.  n_scans = 0 writes only
 * them.  Two launches: a frame index over the list (4 B per (scan, stream) of scratch, allocated at
 * create for max_scans), then one wave64 per stream, serial over its scans. */
typedef struct fmcw_tws_dev_config {   /* 12 words, 48 bytes */
  fmcw_tws_config tws;     /* same fields, same limits as fmcw_tws_create */
  uint32_t n_streams;      /* independent track files, 1..4096 */
  uint32_t max_scans;      /* most scans one call runs, >= 1 (max_scans x n_streams < 2^31); sizes the
                              frame index scratch */
  int32_t device_id;       /* 0..63 */
} fmcw_tws_dev_config;
typedef struct fmcw_tws_dev fmcw_tws_dev;
#define FMCW_TWS_DEV_STATUS_WORDS 2
/* Defaults: fmcw_tws_config_default, 1 stream, 1024 scans, device 0. */
void fmcw_tws_dev_config_default(fmcw_tws_dev_config* cfg);
/* Validates every field before any device access (FMCW_EINVAL, the message names the field, *out is
 * NULL), then FMCW_ENODEV / FMCW_ENOMEM as fmcw_plots_create.  Device memory: 3840 B per stream and
 * 4 B per (scan, stream) of max_scans.  The track files are at power-up when it returns. */
int fmcw_tws_dev_create(const fmcw_tws_dev_config* cfg, fmcw_tws_dev** out);
int fmcw_tws_dev_destroy(fmcw_tws_dev* t);   /* NULL is FMCW_OK */
/* Stream-ordered: every track file back to power-up (no track, best_distance all ones). */
int fmcw_tws_dev_reset(fmcw_tws_dev* t, void* stream);
/* Device pointers only; stream-ordered, allocates nothing, never synchronises.  Arguments are checked
 * before any device access: rec_stride 16 or 32, track_cap >= 1, n_scans <= max_scans, no NULL
 * (recs_dev may be NULL with rec_cap = 0; tracks_dev and counts_dev with n_scans = 0).
 * tracks_dev: n_scans x n_streams x track_cap records; counts_dev: 2 x n_scans x n_streams words;
 * status_dev: FMCW_TWS_DEV_STATUS_WORDS words. */
int fmcw_tws_dev_enqueue(fmcw_tws_dev* t, const void* recs_dev, size_t rec_stride, size_t rec_cap,
                         const uint32_t* n_recs_dev, size_t n_scans, fmcw_track* tracks_dev,
                         size_t track_cap, uint32_t* counts_dev, uint32_t* status_dev, void* stream);
/* Test hook: bounds the workgroups of both kernels (0 = the built-in bound, else the minimum), so that a
 * short list drives one workgroup of the index kernel through several 1024-record tiles and one wave
 * of the tracker through several streams.  Results never depend on it. */
int fmcw_tws_dev_set_grid_for_test(fmcw_tws_dev* t, uint32_t grid);

/* ---- Interference excision: blank or interpolate bursts in the ADC cube before the range FFT ----
 * Another FMCW radar's chirp crossing ours leaves a short burst in some chirps, 30-60 dB above the
 * noise.  A burst in fast time is white in range: it raises the whole range profile of the chirps it
 * hits and, after the Doppler FFT, the whole map, and every CFAR downstream adapts to the raised floor.
 * The exciser finds the burst per chirp against a robust level of the chirp's own power and repairs it
 * before the window and the range FFT: its output is a cube fmcw_enqueue / fmcw_range_ct take as it is.
 *
 * Cube.  [frame][rx][chirp][sample] in any fmcw_in_dtype, as fmcw_enqueue reads it; the repaired cube
 * has the same layout and dtype.  A line is one chirp of one rx of one frame: Ns = n_range complex
 * samples.  Lines are independent.  The specification is exact: every step below is one individually
 * rounded fp32 operation (fl), and no multiplication is contracted with an addition.  Per line:
 *
 * 1. Power.  p[n] = fl(fl(re re) + fl(im im)); re and im are the sample's components converted exactly
 *    to fp32 (from f32, f16 or int16).
 * 2. Level.  m = the k-th smallest p[n] of the line, 0-based ascending rank k = floor(Ns rank_pct / 100),
 *    duplicates counted: an exact order statistic (rank_pct 50 is the median).  p >= +0, so the order of
 *    the values is the order of their bit patterns.
 * 3. Flag.  T = fl(alpha m); f[n] = p[n] > T (strict).  alpha is a power ratio.  m = 0 gives T = 0:
 *    every non-zero sample is flagged.
 * 4. Dilate.  g[n] = OR of f[j] over |j - n| <= guard, j clipped to the line (no wrap, nothing crosses
 *    into the next chirp).
 * 5. Repair every maximal run [a, b] of g by mode:
 *    FMCW_EXCISE_ZERO    0 over the run.
 *    FMCW_EXCISE_INTERP  linear between the neighbours lo = x[a-1] and hi = x[b+1], per component in
 *                        fp32: t = fl(float(n - a + 1) / float(b - a + 2)) (a correctly rounded
 *                        division), d = fl(hi - lo), out = fl(lo + fl(t d)).  A run that touches one end
 *                        of the line holds the one neighbour it has (out = lo, or out = hi); a run that
 *                        covers the whole line is written as zeros.
 *    The fp32 value is written back in the cube's dtype: f16 rounds to nearest even; int16 rounds half to
 *    even and cannot saturate (a convex combination of two int16 values); f32 is written as it is.
 *    Samples outside every run are copied unchanged, bit for bit.
 * 6. Outputs.
 *    out_dev     the repaired cube.  It may equal cube_dev (in place); no other overlap is allowed.  In
 *                place, a line with no flagged sample writes nothing.
 *    mask_dev    nullable: Ns / 32 words per line, bit n % 32 of word n / 32 = g[n].
 *    counts_dev  nullable: one word per line [frame][rx][chirp], the samples with g set.
 *    status_dev  FMCW_EXCISE_STATUS_WORDS (4) words, zeroed by the call itself (a replayed graph starts
 *                from zero) and complete when the call's kernel ends: [0] samples repaired (the sum of the
 *                counts), [1] lines with at least one repaired sample, [2] samples flagged before the
 *                dilation, [3] lines with more than Ns / 2 samples repaired (the level of such a line is
 *                not to be trusted).  Integer atomics only: the words do not depend on the grid.
 * Non-finite samples are outside the specification; the call still ends and writes only inside the
 * caller's buffers. */
#define FMCW_EXCISE_STATUS_WORDS 4
typedef enum { FMCW_EXCISE_ZERO = 0, FMCW_EXCISE_INTERP = 1 } fmcw_excise_mode;
typedef struct fmcw_excise_config {   /* 12 words, 48 bytes */
  uint32_t n_range;            /* Ns: power of two, 64..8192 */
  uint32_t n_doppler;          /* chirps per frame, 1..1024 (need not be a power of two) */
  uint32_t n_rx;               /* 1..64 */
  int32_t in_dtype;            /* fmcw_in_dtype */
  int32_t mode;                /* fmcw_excise_mode */
  uint32_t guard;              /* 0..32 */
  uint32_t rank_pct;           /* 1..99 */
  float alpha;                 /* finite, >= 1 */
  uint32_t max_frames;         /* >= 1; max_frames x n_rx x n_doppler x n_range < 2^32 */
  int32_t device_id;           /* 0..63 */
  uint32_t reserved[2];        /* must be 0 */
} fmcw_excise_config;
typedef struct fmcw_exciser fmcw_exciser;
/* Defaults: 1024, 128, 1 rx, F32, ZERO, guard 4, rank_pct 50, alpha 16.0, max_frames 1, device 0. */
void fmcw_excise_config_default(fmcw_excise_config* cfg);
/* Validates every field before any device access (FMCW_EINVAL, the message names the field, *out is
 * NULL), then FMCW_ENODEV as fmcw_cacfar_create.  An exciser owns no device memory. */
int fmcw_excise_create(const fmcw_excise_config* cfg, fmcw_exciser** out);
int fmcw_excise_destroy(fmcw_exciser* e);   /* NULL is FMCW_OK */
/* Device pointers only; stream-ordered, allocates nothing, never synchronises and keeps no state
 * between calls, so it can be captured into a hipGraph in front of fmcw_enqueue on the same stream and
 * replayed.  One memset of the status words and one launch: every line is read once and written at most
 * once.  Arguments are checked before any device access: status_dev, cube_dev and out_dev non-NULL,
 * n_frames in 1..max_frames, cube_dev and out_dev 16-byte aligned and equal or disjoint. */
int fmcw_excise_enqueue(fmcw_exciser* e, const void* cube_dev, size_t n_frames, void* out_dev,
                        uint32_t* mask_dev, uint32_t* counts_dev, uint32_t* status_dev, void* stream);
/* Test hook: bounds the persistent workgroups, which stride over the lines, so that a small call drives
 * a workgroup through several lines.  0 = the built-in bound (the workgroups resident at once), else
 * min(that bound, grid).  Results never depend on it. */
int fmcw_excise_set_grid_for_test(fmcw_exciser* e, uint32_t grid);

/* ---- TDM-MIMO virtual array: split the chirps by transmitter and time-align the TX slots ----
 * A front end with n_tx transmitters that fire in turn, chirp by chirp, sees n_tx * n_rx virtual
 * channels.  This stage sorts the chirps of fmcw_range_ct's spectrum by transmitter and writes a spectrum
 * of n_tx * n_rx channels and n_d = n_chirps / n_tx chirps, which the bearing estimator, the beamformer
 * and the adaptive weights read unchanged (n_rx' = n_tx * n_rx, n_doppler' = n_d).  The transmitters'
 * chirps are taken at different times: a target's Doppler adds a phase step between the TX blocks of the
 * raw de-interleaved array, which biases the bearing.  FMCW_MIMO_ALIGN_DFT removes it by delaying TX t's
 * sequence by t / n_tx samples, so that every channel is sampled at TX 0's instants.  An object of its
 * own, not part of fmcw_handle / fmcw_config; the reference (one transmitter) has no such stage.
 *
 * Input.   spec[f][k][r][c], complex fp32, exactly as fmcw_range_ct writes it for (n_range, n_chirps,
 *          n_rx); n_chirps = n_tx * n_d.  Chirp c was transmitted by TX c mod n_tx: TX t fires in slot t.
 *          Another firing order permutes the output blocks; that is the caller's business.
 * Output.  out[f][v][r][m], complex fp32, v = t * n_rx + k, m = 0 .. n_d - 1: the layout of a
 *          fmcw_range_ct spectrum for (n_range, n_d, n_tx * n_rx).  With a TX spacing of n_rx elements
 *          the virtual array is the uniform line array the bearing estimator and steering weights assume.
 * Steps.   u_t[m] = spec[f][k][r][m * n_tx + t].
 *          FMCW_MIMO_ALIGN_NONE: out = u_t, a byte-exact copy.
 *          FMCW_MIMO_ALIGN_DFT:  a band-limited circular delay of t / n_tx samples,
 *            U_t[q]      = sum_m u_t[m] exp(-2 pi i q m / n_d)
 *            out[..][m]  = (1 / n_d) sum_q U_t[q] exp(-2 pi i s(q) t / (n_tx n_d)) exp(+2 pi i q m / n_d)
 *            s(q) = q for q < n_d / 2, q - n_d for q >= n_d / 2: the Nyquist bin takes the negative sign.
 *          All arithmetic is fp32.
 * Notes.   TX 0's channels are u_0 up to rounding; with n_tx = 1 the stage is a copy.
 *          The alignment assumes |Doppler| below half the per-TX PRF.  A faster target aliases as it does
 *          in any TDM radar; fmcw_unfold_* is the remedy.
 *          The Doppler window and the MTI canceller are not applied here: the downstream objects apply
 *          theirs.
 *          n_tx is a power of two because fmcw_range_ct needs a power-of-two chirp count: n_tx = 3 is out
 *          of scope. */
typedef enum { FMCW_MIMO_ALIGN_NONE = 0, FMCW_MIMO_ALIGN_DFT = 1 } fmcw_mimo_align;
typedef struct fmcw_mimo_config {   /* 32 bytes */
  uint32_t n_range;            /* as fmcw_config: power of two, 64..8192 */
  uint32_t n_chirps;           /* fmcw_range_ct's n_doppler: power of two, 32..1024 */
  uint32_t n_rx;               /* 1..64; n_tx * n_rx <= 64, the channel limit of the downstream objects */
  uint32_t n_tx;               /* power of two, 1..32; n_d = n_chirps / n_tx >= 32 */
  int32_t align;               /* fmcw_mimo_align */
  uint32_t reserved[2];        /* must be 0 */
  int32_t device_id;           /* 0..63 */
} fmcw_mimo_config;
typedef struct fmcw_mimo fmcw_mimo;
/* Defaults: 1024, 128 chirps, 4 rx, 2 tx, ALIGN_DFT, device 0. */
void fmcw_mimo_config_default(fmcw_mimo_config* cfg);
/* Validates every field before any device access (FMCW_EINVAL, the message names the field, *out is
 * NULL), then FMCW_ENODEV as fmcw_excise_create.  A virtual array owns no device memory. */
int fmcw_mimo_create(const fmcw_mimo_config* cfg, fmcw_mimo** out);
int fmcw_mimo_destroy(fmcw_mimo* m);   /* NULL is FMCW_OK */
/* Device pointers only; stream-ordered, allocates nothing, never synchronises and keeps no state
 * between calls, so it can be captured into a hipGraph after fmcw_range_ct on the same stream and
 * replayed.  One launch: every point is read once and written once.
 * spec_dev: n_frames frames as fmcw_range_ct writes them for (n_range, n_chirps, n_rx), 16-byte aligned.
 * out_dev:  n_frames frames of n_tx * n_rx x n_range x n_d complex fp32 (as many bytes as spec_dev),
 *           16-byte aligned; it must not overlap spec_dev.  Nothing is stored beyond them.
 * n_frames == 0 is FMCW_OK and launches nothing. */
int fmcw_mimo_enqueue(fmcw_mimo* m, const void* spec_dev, size_t n_frames, void* out_dev, void* stream);
/* Test hook: bounds the workgroups of the persistent kernel, whose waves stride over tiles of 1024
 * points, so that a small call drives a workgroup through several tiles, channels and frames.  0 = the
 * built-in bound (the workgroups resident at once), else min(that bound, grid).  Results never depend
 * on it. */
int fmcw_mimo_set_grid_for_test(fmcw_mimo* m, uint32_t grid);

/* ---- Angle resolution: several sources per detection from its channel snapshot ------------
 * fmcw_bearings_* reads one plane wave on a uniform line array.  Two targets in one range-Doppler cell
 * give it one blended bearing, and it cannot use a planar or thinned array or a calibration table.  The
 * resolver scans each record's snapshot (the snaps_dev of fmcw_bearings_enqueue) over a caller-supplied
 * steering table, takes the strongest grid point, cancels it and scans again (matching pursuit), then
 * re-estimates every source against the others (RELAX).  An object of its own, not part of fmcw_handle
 * / fmcw_config; the reference (one receive channel) has no such stage.
 *
 * Steering table.  A[g][k], complex fp32, g = 0 .. n_grid - 1 rows of n_ch entries: the array's response
 *   to a unit source at grid point g, geometry and calibration folded in by the caller.  The object keeps
 *   w[g] = 1 / sum_k |A[g][k]|^2, computed in fp64 and stored as fp32.  fmcw_doa_set_steering rejects a
 *   row whose norm is 0 or not finite; fmcw_doa_set_steering_dev gives such a row w[g] = 0 and reads it as
 *   zeros, so it can never win.  Until a table is set every w[g] is 0.
 *
 * Per record i, s[k] = snaps_dev[i * n_ch + k], r_0 = s:
 *   Stage j = 0 .. k_max - 1:
 *     y_j[g] = sum_k conj(A[g][k]) r_j[k]
 *     B_j[g] = |y_j[g]|^2 w[g]
 *     g_j    = the lowest g at which B_j is largest
 *     the search ends if B_j[g_j] == 0, and for j > 0 if B_j[g_j] < min_rel * B_0[g_0]
 *     a_j = y_j[g_j] w[g_j];   r_{j+1} = r_j - a_j A[g_j][:]
 *   Then relax_passes passes, each over the sources found, in order of discovery: a_j A[g_j][:] is added
 *   back to the residual, g_j and a_j are taken anew from a scan of that residual (the same argmax and
 *   amplitude, no end test), and the new a_j A[g_j][:] is subtracted.
 *   Position.  With refine = 1, on the B of the scan that fixed the source's final g = g_j:
 *     off = 0.5 (B[g-1] - B[g+1]) / (B[g-1] - 2 B[g] + B[g+1]),
 *     off = 0 if that denominator is not negative, or at g = 0 or g = n_grid - 1;  pos = g + off.
 *   With refine = 0, pos = g: for 2-D grids, whose neighbouring indices are not neighbouring angles.
 *   All arithmetic is fp32. */
#define FMCW_DOA_NO_SNAPSHOT 1u   /* the snapshot is all zeros or has a value that is not finite: n_src = 0,
                                     nothing is scanned, total = residual = 0, a spectrum row of zeros */
#define FMCW_DOA_ONE_CH 2u        /* n_ch == 1 */
#define FMCW_DOA_MAX_SRC 4
typedef struct fmcw_doa_src {  /* 16 bytes */
  uint32_t grid;               /* g_j */
  float pos;                   /* g_j + off */
  float amp_re, amp_im;        /* a_j */
} fmcw_doa_src;
typedef struct fmcw_doa {      /* 96 bytes */
  uint32_t frame;              /* the record's cell, copied from cells_dev (zero without it) */
  uint16_t range;
  uint16_t doppler;
  uint32_t flags;              /* FMCW_DOA_* bits */
  uint32_t n_src;              /* sources found, 0 .. k_max */
  float total;                 /* sum_k |s[k]|^2 */
  float residual;              /* sum_k |r[k]|^2 after the last subtraction */
  uint32_t reserved[2];        /* written as 0 */
  fmcw_doa_src src[FMCW_DOA_MAX_SRC];   /* in order of discovery; zeros from n_src on */
} fmcw_doa;
typedef struct fmcw_doa_config {   /* 32 bytes */
  uint32_t n_ch;               /* channels of a snapshot, 1..64 */
  uint32_t n_grid;             /* rows of the steering table: a multiple of 64, 64..1024 */
  uint32_t k_max;              /* most sources per record, 1..4 */
  uint32_t relax_passes;       /* 0..3 */
  float min_rel;               /* in [0, 1): a later source must reach this share of B_0[g_0] */
  uint32_t refine;             /* 0 or 1 */
  uint32_t max_records;        /* most records one call processes, 1..2^31-1 (no scratch depends on it) */
                               /* device memory of a resolver: 16 B x n_ch x n_grid + 4 B x n_grid + 8 KiB */
  int32_t device_id;           /* 0..63 */
} fmcw_doa_config;
typedef struct fmcw_doa_resolver fmcw_doa_resolver;
/* Status words of fmcw_doa_enqueue (n_out_dev). */
#define FMCW_DOA_STATUS_WORDS 2
/* Defaults: 16 channels, 256 grid points, k_max 2, 2 passes, min_rel 0.02, refine 1, max_records 2^20,
 * device 0. */
void fmcw_doa_config_default(fmcw_doa_config* cfg);
/* Validates before any device access (FMCW_EINVAL, the message names the field, *out is NULL), then
 * FMCW_ENODEV / FMCW_ENOMEM as fmcw_bearings_create.  The table starts as zeros. */
int fmcw_doa_create(const fmcw_doa_config* cfg, fmcw_doa_resolver** out);
int fmcw_doa_destroy(fmcw_doa_resolver* d);   /* NULL is FMCW_OK */
/* The steering table from the host: steering_host holds n_grid x n_ch complex fp32 (re, im pairs), row
 * g first.  A row whose norm is 0 or not finite is FMCW_EINVAL (the message names the row) and leaves the
 * object's table as it was.  The upload and the conversion run on `stream`, ordered with the calls enqueued
 * on it before and after; the function returns once steering_host has been read (it waits for `stream`). */
int fmcw_doa_set_steering(fmcw_doa_resolver* d, const float* steering_host, void* stream);
/* The same from device memory (8-byte aligned, the same layout), stream-ordered and capturable: the table
 * need not leave the device.  No row is rejected: see "Steering table" above. */
int fmcw_doa_set_steering_dev(fmcw_doa_resolver* d, const void* steering_dev, void* stream);
/* Device pointers only; stream-ordered, allocates nothing, never synchronises and keeps no state
 * between calls, so it can be captured into a hipGraph after fmcw_bearings_enqueue on the same stream
 * and replayed.  One stream at a time per resolver (its 8 KiB of per-workgroup counts are shared by its
 * calls).
 * snaps_dev: rec_cap snapshots of n_ch complex fp32, 8-byte aligned: fmcw_bearings_enqueue's snaps_dev.
 * cells_dev: NULL, or rec_cap records of cell_stride bytes (16 or 32, else FMCW_EINVAL; 4-byte aligned)
 *            that begin with {uint32 frame; uint16 range; uint16 doppler}: fmcw_bearing, fmcw_det, fmcw_plot.
 * Processes n = min(n_records_dev[0], rec_cap, max_records) records (n is read on the device):
 *   doa_dev[i], i < n (16-byte aligned, room for min(rec_cap, max_records) records); nothing is stored
 *                  beyond them,
 *   spectrum_dev[i * n_grid + g] = B_0[g] as fp32 (4-byte aligned), unless spectrum_dev is NULL,
 *   n_out_dev[0] = n, n_out_dev[1] = the records with FMCW_DOA_NO_SNAPSHOT among them.
 * With n = 0 it writes {0, 0} and touches nothing else. */
int fmcw_doa_enqueue(fmcw_doa_resolver* d, const void* snaps_dev, const void* cells_dev, size_t cell_stride,
                     size_t rec_cap, const uint32_t* n_records_dev, fmcw_doa* doa_dev, float* spectrum_dev,
                     uint32_t* n_out_dev, void* stream);
/* Test hook: bounds the workgroups of the resolver's kernel, whose waves stride over the records, so
 * that a short list drives a workgroup through several records.  0 = the built-in bound (2048), else
 * min(that bound, grid).  Results never depend on it. */
int fmcw_doa_set_grid_for_test(fmcw_doa_resolver* d, uint32_t grid);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* FMCW_H_ */
