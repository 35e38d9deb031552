/*
 * helicon_hip.h — C ABI of libhelicon_hip.so: the MI355X (gfx950) implementation of the
 * denovo3D / HILL-style (twist, rise, Csym) sweep ("Path B" of SURVEY.md).
 *
 * The reference (jianglab/helicon) is pure Python and has no FFI for this path; what a
 * maintainer would bind is the three primitives the sweep composes and the thread-pool loop
 * that drives them.  Each entry point cites the reference interface it replaces
 * (paths relative to the reference's src/helicon/):
 *
 *   hh_simulate            webApps/denovo3D/utils.py:31-189   simulate_helical_projection
 *   hh_power_spectrum      lib/transforms.py:771-820          compute_power_spectra (defaults)
 *   hh_cross_correlation   lib/analysis.py:777-799            cross_correlation_coefficient
 *   hh_cosine_similarity   lib/analysis.py:802-821            cosine_similarity
 *   hh_apply_helical_symmetry  lib/transforms.py:58-165       apply_helical_symmetry
 *   hh_affine_transform_2d lib/transforms.py:315-369          rotate_shift_image (its scipy.ndimage.affine_transform call)
 *   hh_transform_map       lib/transforms.py:168-235          transform_map (Euler ZYZ + scipy.ndimage.map_coordinates, cubic)
 *   hh_low_high_pass_filter_3d  lib/filters.py:349-372        low_high_pass_filter_3d (symmetrize_transform_map's 3-D filter)
 *   hh_map_projections     webApps/denovo3D/utils.py:336-345  generate_xyz_projections
 *   hh_separable_transform_3d  lib/transforms.py:610-660, 714-743  fft_crop, fft_rescale (3-D); plugins/proc3d/fft_resample.py:97-109
 *   hh_warp_affine_2d      lib/transforms.py:238-312          transform_image (its skimage.transform.warp call)
 *   hh_rescale_2d          lib/filters.py:375-412             down_scale, and the app's binning (their skimage rescale call)
 *   hh_helix_moments       lib/analysis.py:645-728            estimate_helix_rotation_center_diameter (closing + moments)
 *   hh_ssim_2d,            lib/analysis.py:487-613            ssim_score / ms_ssim_score / mutual_information_score: the non-cosine
 *   hh_joint_histogram                                        scores of lsq_reconstruct (solver_linear_regression.py:484-524)
 *   hh_align_eval          lib/alignment.py:8-239             align_images (one evaluation of its objective, for many candidates)
 *   hh_nudft2d2            plugins/images2star/calibratepixelsize.py:88-156  fft_resolution_range (its finufft.nufft2d2 call) and
 *                                                             the ring maximum of calibrateMag_process_one_micrograph
 *   hh_set_reference +     webApps/denovo3D/app.py:2455-2523  reconstruction_task (the pool over
 *   hh_sweep[_device]                                         candidates) scoring each candidate by
 *                                                             cc(ref[mask], pwr[mask])
 *                                                             (lib/alignment.py:144-147 idiom)
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success and a
 * negative hh_status otherwise, with a message available from hh_last_error(); nothing calls
 * exit(), and no C++ exception leaves the library: every entry point with a body of its own is a function-try-block
 * that turns std::bad_alloc / std::length_error into HH_ERR_NOMEM and anything else into HH_ERR_INTERNAL (message =
 * what()); no host pointer is retained after a call returns.  Images are C-order float32, ny x nx, with the
 * helical axis along the columns (x); "N" below is the side of a square power-of-two image (the tuned kernels),
 * general sizes: hh_create2.
 * A context is bound to one device and is NOT thread-safe (serialise calls per context).
 */
#ifndef HELICON_HIP_H
#define HELICON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HH_ABI_VERSION 1
#define HH_MAX_UNITS 64

typedef enum hh_status {
  HH_OK = 0,
  HH_ERR_ARG = -1,     /* invalid argument / unsupported size                      */
  HH_ERR_HIP = -2,     /* a HIP runtime call failed                                */
  HH_ERR_STATE = -3,   /* call order (e.g. sweep before set_reference/geometry)    */
  HH_ERR_NOMEM = -4,   /* host or device allocation failed                         */
  HH_ERR_INTERNAL = -5 /* a C++ exception reached the boundary (message: what())   */
} hh_status;

typedef struct hh_ctx hh_ctx;

/* Lattice geometry shared by all candidates of a sweep: the scalar arguments of
 * simulate_helical_projection (utils.py:31-47) other than (twist, rise, csym, rot). */
typedef struct hh_geom {
  double apix;             /* Angstrom / pixel                                             */
  double helical_diameter; /* Angstrom; with n_units == 0 one unit sits at radius d/2      */
  double ball_radius;      /* Angstrom; sigma^2 = ball_radius^2 / ln 2 (utils.py:92)       */
  double tilt;             /* degrees, out-of-plane tilt   (utils.py:166-168)              */
  double psi;              /* degrees, in-plane rotation; applied as -psi like utils.py:167 */
  double dy;               /* Angstrom, shift along the image rows (utils.py:169-170)      */
  int32_t n_units;         /* 0 or 1: the deterministic single-unit branch (utils.py:145-151);
                              >1: units[] gives the asymmetric unit explicitly              */
  int32_t tail_bits;       /* Gaussian support is truncated where a term < 2^-tail_bits
                              (0 selects the default, 24)                                   */
  const double* units;     /* host, n_units x 3: (radius A, azimuth rad, axial offset A) — the
                              reference's r, angle and z draws of utils.py:139-144 before
                              `rot` is added; may be NULL when n_units <= 1                 */
} hh_geom;

/* Per-kernel device time of the sampled launches since the last hh_profile_reset: while
 * profiling is enabled with period k (hh_profile_enable(ctx, k), k >= 1) HIP events are recorded
 * on the context's stream around every launch of every k-th batch of a sweep.  Event records
 * break the back-to-back issue of kernels (about 12 % of a sweep at k = 1), hence the sampling. */
typedef struct hh_profile {
  double ms_first_pass;    /* first pass: k_first_pass / k_first_pass_table (fused: the
                              stand-alone k_column_factors of a sweep's first batch)   */
  double ms_second_pass;   /* k_second_pass, or k_fused_pass (build + row FFT + |F| +
                              log1p + masked moment reduction)                         */
  double ms_finalize;      /* Pearson from moments / several-segment contraction       */
  double ms_centres;       /* k_run_table (run tables of the shared-twist pipelines)   */
  int64_t n_first_pass;    /* launches                                                 */
  int64_t n_second_pass;
  int64_t n_finalize;
  int64_t n_centres;
  int64_t candidates;      /* candidates in the sampled launches                       */
} hh_profile;

int hh_abi_version(void);
int hh_device_count(int* count);
/* Exercises the exception barrier without a device: raises, inside a guarded entry point, an exception of the kind the
 * host code under the ABI can meet — kind 0: std::vector::resize with an absurd element count (std::length_error),
 * 1: an allocation no machine can serve (std::bad_alloc), 2: std::system_error as std::thread raises it, 3: a type
 * outside std::exception — and returns the status the barrier made of it (HH_ERR_NOMEM, HH_ERR_NOMEM, HH_ERR_INTERNAL,
 * HH_ERR_INTERNAL; message from hh_last_error(NULL)); any other kind returns HH_OK.  (The reference is Python: an
 * allocation failure there is a MemoryError the caller can catch, lib/exceptions.py:1-52 — this keeps that property.) */
int hh_selftest_exception(int kind);

/* device: HIP ordinal; n: image side; max_batch: candidates per launch (0 = default).
 * hh_create2 takes the image's rows and columns (utils.py:31-47 and transforms.py:687-704 accept any (ny, nx); the
 * helical axis runs along the columns).  Square power-of-two sides 32 ... 1024 get the tuned kernels (hh_create(n) is
 * hh_create2(n, n)); every other size in [8, 1024]^2 is served by runtime-sized kernels with the same semantics:
 * hh_simulate, hh_power_spectrum, hh_set_reference and the sweeps (candidate lists are swept run by run).  A sweep with
 * tilt / psi, or on a row length nx with a prime factor above 31 (no row-transform plan), takes the direct path: raster and
 * float64 direct transforms per candidate — exact, tens of thousands of candidates per second rather than millions. */
int hh_create(hh_ctx** out, int device, int n, int max_batch);
int hh_create2(hh_ctx** out, int device, int ny, int nx, int max_batch);
void hh_destroy(hh_ctx* ctx);
/* candidates per kernel launch this context was created with (the resolved default). */
int hh_max_batch(const hh_ctx* ctx);
/* Device memory the context holds right now (bytes; its buffers grow with the sweeps it has run and stay until
 * hh_destroy).  parts (may be NULL): {run tables, column factors, two-pass intermediate, several-segment buffers,
 * everything else}.  Typical: C2 (512^2, one 100k launch) 0.11 + 0.004 + 0.27 GB (a list whose runs do not share one
 * rise column: 2.9 GB of column factors); C4 (1024^2) ~7 GB; C5 (64 segments x
 * 20k candidates) ~12 GB of masked spectra.  A spectrum filter (hh_set_spectrum_filter) adds its operators and one
 * batch of candidate planes (at most 128 MB, while a batch holds more than one candidate) to "everything else". */
int64_t hh_memory_bytes(const hh_ctx* ctx, int64_t parts[5]);
/* How hh_sweep cuts a launch of the fused pipeline into workgroups: `runs` runs of `run_len`
 * candidates, `n_kb` ky blocks, `slots` workgroups resident on the device at a time.  The first runs_a runs are cut into
 * groups_a layers of cpw_a candidates each, the others into groups_b layers of cpw_b; out = {runs_a, groups_a, cpw_a,
 * groups_b, cpw_b, layers}.  Pure host arithmetic (the reference has no counterpart: its pool takes one task per candidate,
 * app.py:2473-2476); exported so the plan can be inspected and tested without a device. */
int hh_fused_schedule(int64_t runs, int run_len, int n_kb, int slots, int32_t out[6]);
/* Whether the fused pipeline computes one set of column factors per rise for this list: params = n x 4 float64 in runs of
 * run_len candidates; 1 when there are at least two runs and every run carries run 0's rises, value for value and in the
 * same order (the twist-major grid of itertools.product(twists, rises), csym-major lists of such grids included), else 0.
 * The column factors depend on the rise alone, so such a list needs run_len sets, not n.  Pure host arithmetic. */
int hh_rise_columns_shared(const double* params, int64_t n, int64_t run_len);
/* Subunit index range [-extent, extent] a run's table covers when `rise` is the run's smallest: the largest |i| whose
 * row can pass the window test of any image column (|i| rise <= (nx / 2 + rpx) apix + slack, plus a margin for the
 * device's float32 roundings), never more than the lattice's own ceil(nx apix / rise).  rpx = truncation half-window in
 * pixels, slack = largest |axial offset| of a unit + 1e-3 Angstrom (hh_set_geometry's values).  Pure host arithmetic. */
int64_t hh_table_extent(int nx, double apix, int rpx, double slack, double rise);
/* Where the twist walk at N = 512 keeps its tables: two runs to an entry, [pair][ky][rows][2] complex
 * words, pair = run / 2 and the inner index run & 1, runs counted from the first of the table group (`runs` of them, built
 * by one launch).  out = {offset of (run, ky, row) in complex words from the group's base, words the group occupies,
 * offset of the zeroed word that stands in for the missing partner when `run` is the last of an odd number, else -1}.
 * Pure host arithmetic. */
int hh_pair_table_slot(int64_t runs, int64_t run, int nky, int rows, int ky, int row, int64_t out[3]);
/* Which row kernel hh_sweep takes for an image that is not a power-of-two square, and its launch shape: nx = row length
 * (helical axis), rows_lds = table rows a run keeps in LDS ((2 ceil(nx apix / rise_min) + 1) n_units), kg = table rows
 * one column group may reach (<= 32).  out = {r1, r2, spectrum rows per workgroup, threads per workgroup, LDS buffers
 * for the column factors (2 = double-buffered), dynamic LDS bytes}; r1 = r2 = 0 when nx has no pair of 7-smooth factors
 * <= 32 or the shape does not fit (the Stockham kernel of any radix <= 31 runs then).  Pure host arithmetic, no device. */
int hh_general_plan(int nx, int rows_lds, int kg, int64_t out[6]);
/* ctx may be NULL: returns the message of the last failed hh_create on this thread. */
const char* hh_last_error(const hh_ctx* ctx);

/* Run all later work of this context on `hip_stream` (a hipStream_t, e.g. torch's current
 * stream handle).  NULL means the device's null stream — what torch's default stream is — so
 * work enqueued here is ordered with other work on that stream (e.g. an RCCL all-gather of the
 * scores).  hh_use_own_stream returns to the context's private non-blocking stream (the default). */
int hh_set_stream(hh_ctx* ctx, void* hip_stream);
int hh_use_own_stream(hh_ctx* ctx);

int hh_set_geometry(hh_ctx* ctx, const hh_geom* geom);

/* Score on Fourier-zoomed spectra: compute_power_spectra(..., cutoff_res = (cutoff_y, cutoff_x) Angstrom, output_size =
 * (ony, onx)) of lib/transforms.py:663-713, 771-820 for the experimental image(s) and for every candidate of a sweep.
 * Call it between hh_set_geometry and hh_set_reference: hh_set_reference then takes a mask of ony x onx bytes on the
 * fftshifted zoomed plane (the images keep the context's ny x nx) and every hh_sweep* entry point scores on the zoomed
 * spectrum (any candidate list, tilt / psi / dy included).  ony, onx in [8, 1024], cutoffs > 0; all four arguments zero
 * return the context to the default sampling.  A call that changes the sampling drops the reference (the next sweep
 * reports HH_ERR_STATE until hh_set_reference is called), and so does a later hh_set_geometry with another apix.  Bad
 * arguments return HH_ERR_ARG and change nothing; nothing here touches the device. */
int hh_set_spectrum_zoom(hh_ctx* ctx, int ony, int onx, double cutoff_y, double cutoff_x);

/* Score on low / high-pass filtered spectra: compute_power_spectra(..., low_pass_fraction, high_pass_fraction) of
 * lib/transforms.py:771-820 — low_high_pass_filter (lib/filters.py:314-372) of the spectrum image log1p|F| (or |F|) — for
 * the experimental image(s) and for every candidate of a sweep.  Call it between hh_set_geometry and hh_set_reference.  A
 * fraction outside (0, 1) means that pass is off (the reference's own rule); both off clears the filter.  It combines with
 * hh_set_spectrum_zoom; without a zoom the sweep runs the zoom's product kernel at the identity zoom (the image's own shape
 * and Nyquist), the mask keeps the image's shape.  A call that changes the filter drops the reference (HH_ERR_STATE until
 * the next hh_set_reference).  NaN returns HH_ERR_ARG and changes nothing; nothing here touches the device. */
int hh_set_spectrum_filter(hh_ctx* ctx, double low_pass_fraction, double high_pass_fraction);

/* Score on the phase difference across the meridian as well (lib/transforms.py:823-842, "0 -> even order, 180 -> odd
 * order"): with centre-origin transforms on the scored plane (the zoom's, or the image's shape and Nyquist), F~(u, v) the
 * transform at (-f_y[u], f_x[v]), c = Re(F conj F~) / (|F| |F~|) (0 where that is 0 / 0), q = log1p|F| or |F| and M = q c,
 *     phase score = cosine_similarity(M_exp[mask], M_cand[mask])      (analysis.py:802-821; 0 when a norm is 0)
 *     score       = (1 - weight) * amplitude Pearson + weight * phase score
 * and every hh_sweep* entry point writes that score.  The helix must be centred on row ny / 2 (or hh_geom.dy must say
 * where it is); the subunit's azimuth and an axial shift cancel.  weight in (0, 1] turns the mode on, 0 turns it off; NaN
 * or a value outside [0, 1] returns HH_ERR_ARG and changes nothing.  Call it between hh_set_geometry and hh_set_reference.
 * It combines with hh_set_spectrum_zoom and not with hh_set_spectrum_filter: whichever of the two is set second returns
 * HH_ERR_ARG.  Switching the mode on or off drops the reference (HH_ERR_STATE until the next hh_set_reference); changing
 * only the weight does not.  Nothing here touches the device. */
int hh_set_spectrum_phase(hh_ctx* ctx, double weight);
/* hh_sweep with the phase score on (else HH_ERR_STATE): the combined score, the amplitude Pearson coefficient and the
 * phase score of every candidate, host pointers, [S][g] each; any output may be NULL. */
int hh_sweep_parts(hh_ctx* ctx, const double* params, int64_t g, float* scores, float* amplitude, float* phase);
/* M = q c (map_out) and c (cos_out) of one ny x nx host image on the fftshifted scored plane (the zoom's shape with a
 * zoom set), float64 on the device: the reference side of the phase score.  Either output may be NULL.  Needs
 * hh_set_geometry (the pixel size), not the mode. */
int hh_phase_map(hh_ctx* ctx, const float* image, int log_flag, float* map_out, float* cos_out);

/* Experimental image(s) and mask.  images: host, S x N x N float32; mask: host, N x N bytes on
 * the fftshifted plane (DC at [N/2][N/2]), non-zero = bin takes part in the correlation;
 * log_flag selects log1p(|F|) (transforms.py:807-810).  The library transforms the images on
 * the device and keeps, per segment, the Hermitian half-plane weights and the centred
 * reference spectrum. */
int hh_set_reference(hh_ctx* ctx, const float* images, int n_segments, const uint8_t* mask, int log_flag);

/* Score G candidates.  params: G x 4 float64 (twist deg, rise A, csym, rot deg), csym-major /
 * twist / rise order is the caller's business; scores: S x G float32.  A candidate whose
 * spectrum has zero variance under the mask scores 0 (analysis.py:796-797).
 * hh_sweep takes host pointers and returns after the scores are on the host;
 * hh_sweep_device takes device pointers, enqueues on the context's stream and returns. */
int hh_sweep(hh_ctx* ctx, const double* params, int64_t n_candidates, float* scores);
int hh_sweep_device(hh_ctx* ctx, const double* d_params, int64_t n_candidates, float* d_scores);

/* hh_sweep_device for a caller that also holds the candidate list on the host (h_params, same
 * G x 4 values; may be NULL).  The library reads h_params during the call only, to see how the
 * list is ordered: when it consists of equal-length runs (>= 8) of candidates that share
 * (twist, csym, rot) — the twist-major grid of app.py:2319-2403 — and tilt = psi = 0, each run's
 * column transforms are tabulated once and no candidate is rastered or column-transformed
 * individually; where the table slice and the candidate's column factors fit in LDS the whole
 * candidate is built, row-transformed and reduced inside the compute unit (the "fused" pipeline,
 * DESIGN.md section 4), otherwise the table feeds the two-pass pipeline.  Scores agree with
 * hh_sweep_device to float32 rounding.  hh_sweep does the same analysis on its host list.
 * hh_set_table_path(ctx, mode): 0 = never, 1 = run tables + second pass only, 2 = fused where it
 * fits (default). */
int hh_sweep_device_mirrored(hh_ctx* ctx, const double* d_params, const double* h_params, int64_t n_candidates,
                             float* d_scores);
/* hh_sweep_device_mirrored with a row stride for the scores: segment s of candidate i is written to
 * d_scores[s * ld_scores + i], ld_scores >= n_candidates.  Lets a multi-GPU caller sweep straight into the
 * padded send buffer of its score all-gather (helicon_amd/distributed.py).  h_params may be NULL. */
int hh_sweep_device_strided(hh_ctx* ctx, const double* d_params, const double* h_params, int64_t n_candidates,
                            float* d_scores, int64_t ld_scores);
int hh_set_table_path(hh_ctx* ctx, int mode);
/* Which pipeline the last sweep of this context ran: 0 = per-candidate raster + column transform +
 * second pass, 1 = run tables + second pass, 2 = fused, 3 = zoomed spectra (hh_set_spectrum_zoom),
 * 4 = filtered spectra (hh_set_spectrum_filter, with or without a zoom), 5 = amplitude and phase score
 * (hh_set_spectrum_phase, with or without a zoom). */
int hh_last_first_pass(const hh_ctx* ctx);
/* How many sets of column factors the last sweep of this context computed on the fused pipeline: the run length when
 * every run shares one rise column (hh_rise_columns_shared) and a launch holds whole runs, the number of candidates
 * swept by the fused pipeline otherwise, 0 when the sweep ran another pipeline. */
int64_t hh_last_factor_sets(const hh_ctx* ctx);
/* How the fused pipeline walks a list that has one set of column factors per rise.  1 = rises: a
 * workgroup owns (run, ky block), keeps the run's table slice and fetches a factor set per candidate.  2 = twists: a
 * workgroup owns (rise, ky block), keeps the rise's factor set, and each wavefront fetches its own ky row of the next
 * run's table per candidate (no workgroup barrier in the candidate loop; sizes up to 512).  0 = auto (default): twists
 * where a launch holds whole runs, the compute unit holds as many twist-walking workgroups as rise-walking ones (the
 * table rows are double-buffered: 16 bytes per table row and ky instead of 8) and the schedule's estimate is not above
 * the rise walk's; rises otherwise, and always with several segments (their q stores were measured slower on the twist
 * walk).  A forced 2 that cannot run (per-candidate factors, N = 1024, the footprint) falls
 * back to 1.  Scores do not depend on the walk, bit for bit, under modes 1 and 2.
 * 3 = packed: the twist walk at n = 512 with ONE row transform for the two runs of a pair ("One
 * transform per pair").  It needs a centrosymmetric lattice (hh_lattice_centrosymmetric), one segment and the pair walk;
 * where one of them fails it is mode 2.  The two runs of a pair share one transform's roundings, so a score depends, in
 * its last float32 bits, on the run it is paired with: the same list gives the same bits whatever the workgroups' cut
 * (pairs are counted from the first run of a table group), another list or shard may not.  Mode 0 takes the packed form
 * wherever it takes the twist walk and the packed form can run; a caller who needs scores that do not depend on the
 * list forces 2.
 * hh_last_fused_walk: 2 when every fused launch of the last sweep walked twists (packed or not), 1 when one of them walked
 * rises, 0 when the sweep ran another pipeline.  hh_last_fused_packed: 1 when every fused launch of the last sweep walked
 * twists with one transform per pair, else 0. */
int hh_set_fused_walk(hh_ctx* ctx, int mode);
int hh_last_fused_walk(const hh_ctx* ctx);
int hh_last_fused_packed(const hh_ctx* ctx);
/* Whether a sweep of `params` (count x 4 float64: twist, rise, csym, rot) under geometry `geom` on ny x nx images simulates
 * a lattice that is centrosymmetric about the pixel (ny/2, nx/2): one unit at azimuth 0 and axial offset 0, no tilt, psi or
 * dy, no ball within reach of image row 0 (radius / apix + truncation half-window + 1 <= ny / 2), and rot = 0 on every
 * candidate; csym is free.  Rows of the column-transformed image are then Hermitian about column nx/2 but for column 0.
 * 1 / 0, HH_ERR_ARG on a bad argument.  Pure host arithmetic: the geometry and list part of the packed walk's gate. */
int hh_lattice_centrosymmetric(const hh_geom* geom, int ny, int nx, const double* params, int64_t count);
/* Test and tuning hook: the twist walk cuts every rise's runs into workgroups of runs_per_workgroup runs (the last one
 * takes what is left) instead of the cut of hh_fused_walk_choice; 0 (default) = the schedule's own cut.  The choice of
 * the walk is not affected. */
int hh_set_fused_piece(hh_ctx* ctx, int runs_per_workgroup);
/* Dynamic LDS bytes of one workgroup of the fused pass: walk 1 = panel + one table slice (8 ky x rows_lds x 8 B) + two
 * factor sets (kg x n x 4 B + (n / 4 + 4) x 4 B each), walk 2 = panel + two slices + one set; 0 for walk 2 where the
 * size has no twist walk (n = 1024).  Pure host arithmetic. */
int64_t hh_fused_lds_bytes(int n, int rows_lds, int kg, int walk);
/* The walk a launch of `runs` whole runs of `run_len` candidates takes under `mode` (hh_set_fused_walk) when the device
 * holds slots_rises rise-walking and slots_twists twist-walking workgroups at a time (0: the twist walk cannot run), and
 * both schedules: out = {walk (1 or 2), then for the rise walk and for the twist walk: the model's launch length in
 * candidates and hh_fused_schedule's six numbers — for the twist walk with the roles swapped (runs_a counts rises, cpw
 * counts runs)}.  Pure host arithmetic. */
int hh_fused_walk_choice(int64_t runs, int run_len, int n_kb, int slots_rises, int slots_twists, int mode, int64_t out[15]);
/* The fused pass's shape for a sweep of this context (geometry and reference set) whose smallest rise is rise_min:
 * out = {table rows staged per ky, table rows per group of four columns, LDS bytes of the rise walk, of the twist walk,
 * workgroups a compute unit holds of the rise walk, of the twist walk (the first six are zero when the fused pass does
 * not fit), compute units of the device, ky blocks the reference's mask touches}. */
int hh_fused_walk_footprint(hh_ctx* ctx, double rise_min, int64_t out[8]);
/* Which row kernel the last sweep of a general-size context (hh_create2, not a power-of-two square) ran, read-only:
 * out = {R1, R2, dynamic LDS bytes} for the two-step kernel of the pair nx = R1 R2, {0, 0, LDS bytes} for the Stockham
 * kernel, {0, 0, 0} for the float64 direct path (a row length with a prime factor above 31, tilt / psi, a launch that
 * does not fit the LDS) and for any other context.  A list swept in several batches reports its last batch. */
int hh_last_row_kernel(const hh_ctx* ctx, int32_t out[3]);

/* Pre-sweep image preparation on the device.
 * hh_low_high_pass_filter: helicon.low_high_pass_filter (lib/filters.py:314-372) for one N x N float32 image
 * (host in, host out): Gaussian low pass exp(-ln2 R^2 / lp^2) and / or high pass 1 - exp(-ln2 R^2 / hp^2),
 * R = radius as a fraction of Nyquist; a fraction outside (0, 1) switches that filter off.
 * hh_threshold_data: helicon.threshold_data (lib/filters.py:283-311) for n float32 values (host in, host out):
 * out = clip(data, t, None) - t in float32 with t = max(data) * (float)thresh (use_fraction != 0) or t = (float)thresh.
 * The maximum is np.max's: of negative values the one nearest zero, -0.0 where that is the largest value (+0.0 counts
 * as above -0.0), NaN when any element is NaN — every output is then NaN, as from NumPy.  With a number for t a NaN
 * element stays NaN at its own position and nowhere else. */
int hh_low_high_pass_filter(hh_ctx* ctx, const float* image, double low_pass_fraction, double high_pass_fraction,
                            float* out);
int hh_threshold_data(hh_ctx* ctx, const float* data, int64_t n, int use_fraction, double thresh, float* out);

/* arg-max with ties resolved to the lowest index (np.argmax); NaN never wins. */
int hh_argmax(const float* scores, int64_t n, int64_t* index);

/* The same rule for device-resident scores: row r (a segment of a sweep's S x G output, or one rank's
 * block of an all-gathered buffer) is d_scores[r * ld .. r * ld + n), ld = 0 meaning n.  One reduction kernel on
 * the context's stream writes n_rows indices to d_index (device; NULL = a buffer of the context); when h_index
 * is not NULL they are also copied to the host and the call returns after they have arrived, otherwise the
 * call is asynchronous.  Replaces pulling S x G floats to the host for S indices. */
int hh_argmax_device(hh_ctx* ctx, const float* d_scores, int64_t n_rows, int64_t n, int64_t ld, int64_t* d_index,
                     int64_t* h_index);

/* The multi-GPU sweep's only collective for a caller without a host framework (the
 * reference has no distributed code, its candidates are pool tasks: app.py:2473-2476).  One process per GPU, one
 * context each.  RCCL is loaded with dlopen("librccl.so.1") on first use, so a single-GPU user never needs it.
 *   hh_comm_unique_id   rank 0 fills 128 bytes (ncclUniqueId) and hands them to the other ranks by any means;
 *   hh_comm_init        every rank, collectively: a communicator of `world` ranks bound to this context;
 *   hh_allgather        every rank contributes `count` floats from d_send; d_recv receives world x count floats in
 *                       rank order; enqueued on the context's stream, i.e. ordered behind the sweep that produced
 *                       d_send (hh_sweep_device_strided into a NaN-padded buffer: helicon_amd/distributed.py is the
 *                       same step with torch.distributed) and ahead of hh_argmax_device on d_recv;
 *   hh_comm_destroy     also done by hh_destroy. */
int hh_comm_unique_id(void* id128);
int hh_comm_init(hh_ctx* ctx, int rank, int world, const void* id128);
int hh_allgather(hh_ctx* ctx, const float* d_send, int64_t count, float* d_recv);
int hh_comm_destroy(hh_ctx* ctx);

/* One simulated projection (host, N x N float32) for params[4] = (twist, rise, csym, rot). */
int hh_simulate(hh_ctx* ctx, const double* params, float* image_out);

/* Amplitude spectrum of one host image: pwr_out (N x N, fftshifted, min-max normalised as
 * transforms.py:817) and phase_out (N x N, radians; may be NULL). */
int hh_power_spectrum(hh_ctx* ctx, const float* image, int log_flag, float* pwr_out, float* phase_out);

/* Pearson / cosine of two host vectors (float32 or float64), reduced on the device in float64
 * with the reference's two-pass (means, then centred sums) order of operations. */
int hh_cross_correlation(hh_ctx* ctx, const float* a, const float* b, int64_t n, double* out);
int hh_cosine_similarity(hh_ctx* ctx, const float* a, const float* b, int64_t n, double* out);
int hh_cross_correlation_f64(hh_ctx* ctx, const double* a, const double* b, int64_t n, double* out);
int hh_cosine_similarity_f64(hh_ctx* ctx, const double* a, const double* b, int64_t n, double* out);

/* The resampling step of helicon.rotate_shift_image (lib/transforms.py:315-369; used by the app's
 * auto_horizontalize, webApps/denovo3D/utils.py:410, 423): scipy.ndimage.affine_transform(data, matrix, offset,
 * order = 1, mode = "constant") of one ny x nx float32 image — out[y][x] = bilinear sample of data at
 * matrix (y, x) + offset (row-major 2 x 2 matrix, (y, x) offset), 0 where the sample point leaves [0, n - 1].
 * The caller builds matrix / offset from the angle, shifts and rotation centre exactly as the reference does
 * (helicon_amd.rotate_shift_image shows it).  Context-free: errors are read with hh_last_error(NULL). */
int hh_affine_transform_2d(int device, const float* data, int ny, int nx, const double matrix[4], const double offset[2],
                           float* out);

/* The same with order = 3 (auto_horizontalize's last step, webApps/denovo3D/utils.py:420-423:
 * rotate_shift_image(order = 3)): float64 B-spline prefilter with mirror boundaries, 4 x 4 cubic taps, 0 where the sample
 * point leaves [0, n - 1]. */
int hh_affine_transform_2d_cubic(int device, const float* data, int ny, int nx, const double matrix[4], const double offset[2],
                                 float* out);

/* ---- pre-sweep image preparation that is scikit-image in the reference -------------------------
 * scikit-image is not installed beside the reference in the build environment: these four are pinned BY DERIVATION
 * (oracle/prep.py restates scikit-image 0.25's call sequences on the installed SciPy / in NumPy; csrc/image_prep.inc).
 * `data` / `out` are host rows x cols images, float32 (is_f64 = 0) or float64 (is_f64 = 1) — scikit-image computes in the
 * image's own floating type, and so do these.  Context-free: errors are read with hh_last_error(NULL).
 *
 * hh_warp_affine_2d — skimage.transform.warp(image, inverse_map, order, mode = "constant", cval, clip) of a 2-D image
 * through its fast path, what helicon.transform_image (lib/transforms.py:238-312) calls: inverse_matrix is the row-major
 * 3 x 3 matrix that maps OUTPUT (col, row, 1) to INPUT (col, row, w) (helicon_amd.transform_image composes it as the
 * reference does); order 0 (nearest) or 1 (bilinear); a sample outside the image is cval; clip != 0 clips the result to the
 * input's range (pixels equal to a cval outside that range keep it). */
int hh_warp_affine_2d(int device, const void* data, int is_f64, int rows, int cols, const double inverse_matrix[9], int order,
                      double cval, int clip, void* out);

/* hh_rescale_2d — skimage.transform.rescale / resize(image, (out_rows, out_cols), order, mode = "reflect",
 * anti_aliasing, clip), what the app's binning (webApps/denovo3D/app.py:1911-1922) and helicon.down_scale
 * (lib/filters.py:375-412) call: a Gaussian of sigma = max(0, (rows / out_rows - 1) / 2) per axis (scipy.ndimage.gaussian_filter,
 * truncate 4, mirror boundaries) when anti_aliasing != 0, then scipy.ndimage.zoom(order, mode = "mirror", grid_mode = True)
 * — order 3 on the float64 mirror-prefiltered image, order 1 on the image itself —, then the clip to the input's range.
 * The caller computes (out_rows, out_cols) = max(round(scale * shape), 1) as rescale does. */
int hh_rescale_2d(int device, const void* data, int is_f64, int rows, int cols, int out_rows, int out_cols, int order,
                  int anti_aliasing, int clip, void* out);

/* hh_helix_moments — the numeric part of helicon.estimate_helix_rotation_center_diameter (lib/analysis.py:645-728):
 * mask = skimage.morphology.closing(data > threshold, mode = "ignore") (3 x 3 cross: a dilation, then an erosion, both
 * ignoring what lies outside the image), then _weighted_params over the mask in float64 with w = I - min_mask(I) + 1e-8.
 * out = {pixels in the mask, c_y, c_x, i_yy, i_xx, i_xy, first mask row, last mask row}; with an empty mask out[0] = 0 and
 * the rest is not meaningful. */
int hh_helix_moments(int device, const void* data, int is_f64, int rows, int cols, double threshold, double out[8]);

/* hh_ssim_2d — skimage.metrics.structural_similarity(a, b, data_range=...) with its defaults (7 x 7 uniform window, sample
 * covariance, K1 = 0.01, K2 = 0.03) of two float32 images, what helicon.ssim_score and ms_ssim_score call (lib/analysis.py:
 * 487-582; the "ssim" / "ms_ssim" / "composite" scores of lsq_reconstruct, solver:484-524): the mean of the SSIM map over the
 * image without its 3-pixel rim, float32 arithmetic in numpy's operation order, the mean in float64.  rows, cols >= 7. */
int hh_ssim_2d(int device, const float* a, const float* b, int rows, int cols, double data_range, double* out);

/* hh_joint_histogram — the counts of np.histogramdd([a, b], bins) for skimage.metrics.normalized_mutual_information
 * (helicon.mutual_information_score, lib/analysis.py:585-613): edges_a / edges_b are the caller's np.linspace(min, max,
 * bins + 1); hist: int64 [bins][bins], first index = a's bin. */
int hh_joint_histogram(int device, const float* a, const float* b, int64_t n, const double* edges_a, const double* edges_b, int bins,
                       int64_t* hist);

/* helicon.transform_map (lib/transforms.py:168-235; the reference's task function resamples the symmetrised map with
 * it when tilt / psi / dy are not zero, pipeline.py:430-432): data is host float32 [shape[0]][shape[1]][shape[2]] (z, y, x);
 * the sampling grid, centred on voxel (n // 2), is scaled, rotated by the intrinsic ZYZ Euler angles (rot, tilt, psi;
 * degrees) and shifted by (dx, dy, dz), and the volume is resampled as scipy.ndimage.map_coordinates(order = 3) does:
 * float64 B-spline prefilter with mirror boundaries, 4 x 4 x 4 cubic taps, 0 where the sample point leaves the volume.
 * out: float32, same shape.  Context-free: errors are read with hh_last_error(NULL). */
int hh_transform_map(int device, const float* data, const int32_t shape[3], double scale, double rot_degree, double tilt_degree,
                     double psi_degree, double dx, double dy, double dz, float* out);

/* Helical symmetrisation of a 3-D map (transforms.py:58-165): data is host float32
 * [in_shape[0]][in_shape[1]][in_shape[2]] (z, y, x); new_size / new_apix as in the reference (pass the
 * input's own shape / apix for "unchanged").  out receives out_shape[0..2] float32 voxels — the
 * requested size, or its even-cropped version when the reference's final slice applies
 * (transforms.py:158-164); call with out == NULL to query out_shape only.  kernel_ms (may be NULL)
 * returns the device time of the gather kernel.  Context-free: errors are read with
 * hh_last_error(NULL). */
int hh_apply_helical_symmetry(int device, const float* data, const int32_t in_shape[3], double apix,
                              double twist_degree, double rise_angstrom, int csym, double fraction,
                              const int32_t new_size[3], double new_apix, float* out, int32_t out_shape[3],
                              double* kernel_ms);

/* The 3-D branch of helicon.low_high_pass_filter (lib/filters.py:349-372), which the app's symmetrize_transform_map runs
 * on every map it resamples to a coarser pixel (webApps/denovo3D/utils.py:361-366): Re ifftn(fftn(x) * fftshift(filter)),
 * the Gaussian low pass exp(-f2 R^2) and / or high pass 1 - exp(-f2 R^2), f2 = ln 2 / fraction^2, R on the reference's
 * centred float32 grid.  Computed as three 1-D circulant operators (one per axis) on the exact-f32 MFMA, for any side.
 * data / out: host float32 [shape[0]][shape[1]][shape[2]] (z, y, x); every side in [2, 1024]; a fraction outside (0, 1)
 * is ignored, as in the reference.  Context-free: errors are read with hh_last_error(NULL). */
int hh_low_high_pass_filter_3d(int device, const float* data, const int32_t shape[3], double low_pass_fraction,
                               double high_pass_fraction, float* out);

/* The three axis projections of a map (generate_xyz_projections, webApps/denovo3D/utils.py:336-345): out_x[nz][ny] =
 * sum over x, out_y[nz][nx] = sum over y, out_z[ny][nx] = sum over z, or over the slab z in [slab_begin, slab_end) when
 * slab_begin >= 0 (the amyloid view; the caller resolves the reference's Python slice).  float64 running sums, float32
 * results.  Context-free: errors are read with hh_last_error(NULL). */
int hh_map_projections(int device, const float* data, const int32_t shape[3], int32_t slab_begin, int32_t slab_end, float* out_x,
                       float* out_y, float* out_z);

/* Fourier resampling of a 3-D map or a 2-D image: what fft_rescale's 3-D branch (lib/transforms.py:714-743), fft_crop
 * (:610-660) and proc3d --fft_resample (plugins/proc3d/fft_resample.py:97-109) have in common.  One complex operator per
 * axis, op[a] = op_re[a] + i op_im[a], host float32 [out_shape[a]][in_shape[a]] row-major, is applied along z, then y,
 * then x on the exact-f32 MFMA; op_im[a] NULL: a real operator; both NULL: the identity (the axis is skipped and keeps
 * its side).  The caller builds the operators in float64 and rounds them once (helicon_amd/fft_resample.py).  The last
 * pass applies the epilogue to the complex product c: 0 store (out0 = Re c, out1 = Im c), 1 abs (out0 = |c| * scale),
 * 2 real (out0 = Re c * scale; the imaginary part is not computed); out1 is read under store only.
 * data: host float32 [in_shape]; out0 / out1: host float32 [out_shape]; every side, in and out, in [1, 1024].
 * Context-free: errors are read with hh_last_error(NULL). */
int hh_separable_transform_3d(int device, const float* data, const int32_t in_shape[3], const int32_t out_shape[3],
                              const float* const op_re[3], const float* const op_im[3], int epilogue, double scale, float* out0,
                              float* out1);
/* device-event milliseconds of the last hh_separable_transform_3d call's passes (the copies of the map excluded) */
int hh_separable_transform_kernel_ms(double* ms);

int hh_synchronize(hh_ctx* ctx);

int hh_profile_enable(hh_ctx* ctx, int on);
int hh_profile_reset(hh_ctx* ctx);
int hh_profile_get(hh_ctx* ctx, hh_profile* out);

/* Profiling aid: one launch that moves `bytes` (rounded down to whole MiB) with the sweep's
 * read shape (mode 0: contiguous 16-byte-per-lane block reads of k_second_pass) or write shape
 * (mode 1: whole 128-byte lines, 8 lanes each, one line per ky block, as k_first_pass stores them), so rocprofv3's FETCH_SIZE / WRITE_SIZE can be calibrated on a
 * known byte count for exactly these access patterns. */
int hh_calibrate_traffic(hh_ctx* ctx, int mode, int64_t bytes);

/* Algorithmic HBM bytes per candidate, B_alg(N) = 4 N^2 + 16 N (N/2 + 1). */
int64_t hh_algorithmic_bytes(int n);

/* ---------------------------------------------------------------------------------------------------------------
 * Path A, first slice: the reference's shipped scorer (sparse least squares + cosine) with a matrix-free
 * nearest-neighbour projector.  Replaces, for interpolation="nn": build_A_data_matrix
 * (webApps/denovo3D/solver_linear_regression.py:1304-1654), build_A_helical_sym_matrix (:847-1298) and the
 * scipy.sparse.linalg.lsmr calls behind scipy.optimize.lsq_linear (:258-269).  The bounded trust-region iteration,
 * the positivity rule and the score stay on the host: helicon_amd/solver.py (lsq_reconstruct, :31-547).
 * An hh_pa is one candidate's implicit system: rows = [projection rays with at least one sample in the cylinder,
 * in the reference's (symmetry operation, k, j) order] + [symmetry constraints x_i - x_j = 0]; unknowns = voxels of
 * the cylinder in C-order rank.  Vectors cross this boundary as host float64 arrays. */
typedef struct hh_pa hh_pa;
typedef struct hh_pa_params {
  double scale2d_to_3d, twist_degree, rise_pixel;
  int32_t csym;
  double tilt_degree, psi_degree, dy_pixel;
  int32_t reconstruct_diameter_2d_pixel, reconstruct_length_2d_pixel, reconstruct_diameter_3d_pixel,
      reconstruct_diameter_3d_inner_pixel, reconstruct_length_3d_pixel;
  int64_t min_projection_lines;   /* stop adding symmetry operations once the data rows exceed this (solver:1647) */
  int64_t min_sym_pairs;          /* symmetry rows wanted (solver:1275); 0 = no symmetry block */
  int32_t interpolation;          /* 0 = "nn" (solver:1511-1553, 1142-1298), 1 = "linear" (solver:1414-1503, 910-1140:
                                     trilinear weights, rays recomputed in every product, 16-entry symmetry rows) */
  int32_t fsc_mode, fsc_half;     /* half sets of lsq_reconstruct's fsc_test (split_A_b, solver:175-203): fsc_half 0 = all
                                     data rows, 1 / 2 = the rows of the first / second half of the pixel ids under
                                     fsc_mode 2 (every second id), 3 (lower / upper half), >= 4 (outer / middle thirds),
                                     1 (the ids listed in fsc_ids / the others: the caller's random split, :186-189) */
  int32_t n_fsc_ids;              /* fsc_mode 1 only: number of pixel ids (k * D2d + j) in the first half ... */
  const int32_t* fsc_ids;         /* ... and the ids, any order; read during the create call only */
} hh_pa_params;
int hh_pa_create(hh_pa** out, int device, const float* image, int ny, int nx, const hh_pa_params* params);
void hh_pa_destroy(hh_pa* pa);
const char* hh_pa_last_error(const hh_pa* pa);
/* dims = {unknowns, data rows, symmetry rows, symmetry operations used} */
int hh_pa_dims(const hh_pa* pa, int64_t dims[4]);
/* b (pixel value of every data row) and b_pid (k * D2d + j), solver:1548-1549 */
int hh_pa_get_rhs(const hh_pa* pa, float* b, int32_t* b_pid);
/* y = Op x and g = Op^T y for Op = [A diag(d); diag(root)] (d, root may be NULL: Op = A = [A_data; A_hsym]);
 * y has data rows + symmetry rows (+ unknowns when root is given) entries. */
int hh_pa_matvec(hh_pa* pa, const double* x, const double* d, const double* root, double* y);
int hh_pa_rmatvec(hh_pa* pa, const double* y, const double* d, const double* root, double* g);
/* scipy.sparse.linalg.lsmr(Op, rhs, atol, btol, conlim, maxiter) with all vectors on the device;
 * info = {istop, itn}, norms = {normr, normar} (either may be NULL). */
int hh_pa_lsmr(hh_pa* pa, const double* rhs, const double* d, const double* root, double atol, double btol, double conlim,
               int maxiter, double* x_out, int info[2], double norms[2]);


/* compute_power_spectra(data, apix, cutoff_res, output_size, log) with a Fourier-space zoom (lib/transforms.py:771-820 over
 * fft_rescale, :663-713): the image's transform at ony x onx frequencies fftfreq(on) * 2 * apix / cutoff_res, as the
 * direct sum finufft.nufft2d2(eps=1e-6) approximates, float64; (-1)^(u+v), fftshift, |F| (log1p when log_flag), min-max
 * normalisation; phase_out (may be NULL) = angle of the shifted transform.  image: ny x nx host float32; outputs ony x onx. */
int hh_power_spectrum_zoom(int device, const float* image, int ny, int nx, int ony, int onx, double apix, double cutoff_y,
                           double cutoff_x, int log_flag, float* pwr_out, float* phase_out);

/* ---------------------------------------------------------------------------------------------
 * Path A for MANY candidates at once (round 3): K candidates of one image and one reconstruction box — the K tasks the
 * reference's thread pool runs one by one (webApps/denovo3D/app.py:2473-2476 -> pipeline.py:351-404 ->
 * solver_linear_regression.py:31-547) — set up together and solved together on the device: every LSMR iteration and
 * every step of scipy.optimize.lsq_linear's trust-region-reflective loop (solver_linear_regression.py:258-269) is one
 * launch for all K; the host only reads "is anyone still iterating?".  Nearest-neighbour projector (params[i]
 * .interpolation == 0); the candidates differ in twist / rise / csym / tilt / psi / dy / fsc half and share the
 * 2-D region, the 3-D box and the row targets' meaning. */
typedef struct hh_pab hh_pab;
int hh_pab_create(hh_pab** out, int device, const float* image, int ny, int nx, const hh_pa_params* params, int count);
/* hh_pab_create with flags (0: the same).  The trilinear products of hh_pab_create keep two whole planes of the cylinder in
 * LDS and refuse a box where those and the disc's index table pass 150 KB (D2d ~ 100).  HH_PAB_ALLOW_BANDED: such a box takes
 * the banded form (csrc/path_a_banded.inc: each cell layer cut into bands of disc rows that fit; the same entries in float64,
 * A^T y still in integer fixed point); HH_PAB_FORCE_BANDED: every box does, cut into at least three bands (for tests).
 * tilt = psi = 0 as the other slice-major forms. */
#define HH_PAB_ALLOW_BANDED 1
#define HH_PAB_FORCE_BANDED 2
int hh_pab_create_ex(hh_pab** out, int device, const float* image, int ny, int nx, const hh_pa_params* params, int count, int flags);
/* the form of the products an hh_pab uses (or HH_ERR_ARG) */
#define HH_PAB_FORM_GENERAL 0   /* nearest neighbour, int32 map gathered from L2 (any tilt / psi, or slices beyond 60 KB) */
#define HH_PAB_FORM_SLICED 1    /* nearest neighbour, one z slice per workgroup in LDS */
#define HH_PAB_FORM_LDS 2       /* trilinear, two planes per workgroup in LDS */
#define HH_PAB_FORM_FACTORED 3  /* trilinear, separable form (csrc/path_a_factored.inc) */
#define HH_PAB_FORM_BANDED 4    /* trilinear, bands of disc rows (csrc/path_a_banded.inc) */
int hh_pab_product_form(const hh_pab* pab);
void hh_pab_destroy(hh_pab* pab);
const char* hh_pab_last_error(const hh_pab* pab);
/* dims = {candidates, unknowns, total data rows, total symmetry rows, device bytes held};
 * rows (may be NULL): [count][3] = {data rows, symmetry rows, symmetry operations used} */
int hh_pab_dims(const hh_pab* pab, int64_t dims[5], int64_t* rows);
/* b and pixel id (k * D2d + j) of candidate c's data rows (solver:1548-1549) */
int hh_pab_get_rhs(const hh_pab* pab, int c, float* b, int32_t* b_pid);
/* the symmetry rows of candidate c as voxel-rank pairs (row: x_i - x_j = 0; build_A_helical_sym_matrix,
 * solver:1142-1298) in the reference's row order; out: [symmetry rows][2] */
int hh_pab_get_pairs(hh_pab* pab, int c, int32_t* out);
/* lsq_linear(A_c, b_c, bounds = positive[c] ? (0, max b_c) : none, tol, max_iter, lsmr_maxiter, lsmr_tol="auto") for
 * every candidate; x -> float32; score = cosine(A_data x [clipped at 0 when clip[c]], b) (solver:484-530).
 * x_out: [count][unknowns] float32 or NULL; scores: [count]; info: [count][5] = {lsq_linear status, trust-region
 * iterations, LSMR solves, LSMR iterations, of which in the first (unconstrained) solve} or NULL. */
int hh_pab_solve(hh_pab* pab, const int32_t* positive, const int32_t* clip, double tol, int max_iter, int lsmr_maxiter,
                 float* x_out, double* scores, int32_t* info);
/* Host-only check of the trilinear products' ray arithmetic (csrc/path_a_linear.inc): the coordinates of every sample of
 * every ray under every symmetry operation of candidate *params (tilt = psi = 0), once as pa_coords computes them
 * (back_project_2d_coords_to_3d_coords + solver:1389-1394, 1576-1581) and once with the per-ray part hoisted as the product
 * kernels do; out = {samples, samples that differ, ray and sample of the first, and — with device >= 0, else -1 — the same
 * two counts by that device's arithmetic, then the samples whose cell decision differs there, -1}.  device < 0: host only. */
int hh_pab_check_ray_arithmetic(const hh_pa_params* params, int ny, int nx, int device, int64_t out[8]);
/* y = A_c x and g = A_c^T y for candidate c through the product kernels the solve uses (A_c = [A_data; A_hsym], the matrix
 * build_A_data_matrix / build_A_helical_sym_matrix return, solver:1304-1654, 847-1298; rows in the reference's order):
 * x, g: [unknowns], y: [data rows + symmetry rows], host float64.  For the parity tests; not during a solve. */
int hh_pab_matvec(hh_pab* pab, int c, const double* x, double* y);
int hh_pab_rmatvec(hh_pab* pab, int c, const double* y, double* g);
/* The scikit-learn models of solve_equations (solver_linear_regression.py:270-342: ElasticNet — the reference app's default,
 * app.py:555-558 —, Lasso, Ridge, LinearRegression, all with fit_intercept = True) for every candidate: the minimiser of
 *   (1 / 2m) || (b - mean b) - (A - 1 mu^T) w ||^2 + alpha[c] l1_ratio |w|_1 + alpha[c] (1 - l1_ratio) / 2 |w|^2,  w >= 0 where positive[c]
 * (mu = column means of A, m = rows; ridge_form: alpha[c] / m, the scaling of sklearn's Ridge) by accelerated proximal gradient
 * on the implicit operator, float64; x -> float32 and the cosine score as hh_pab_solve.  The reference's solvers visit the
 * coordinates in a random order and stop loosely, in float32: for l1_ratio < 1 (or full column rank) the minimiser is unique and
 * this is it.  tol: max |w_new - w| <= tol max |w_new|.  info: [count][3] = {iterations, converged, non-zero coefficients};
 * objective: [count] value of the function above at w; x_out, info, objective may be NULL.  Needs tilt = psi = 0 (any form of
 * the products: sliced, general nearest neighbour, or a trilinear form). */
int hh_pab_solve_prox(hh_pab* pab, const int32_t* positive, const int32_t* clip, const double* alpha, double l1_ratio, int ridge_form,
                      double tol, int max_iter, float* x_out, double* scores, int32_t* info, double* objective);
/* counters of the last hh_pab_solve: {kernel launches, host synchronisations, LSMR iterations queued, failures of the
 * solver's self-check (every workgroup of a launch saw the per-candidate state the previous launch wrote; must be 0)} */
int hh_pab_counters(const hh_pab* pab, int64_t out[4]);

/* ---------------------------------------------------------------------------------------------
 * Helical symmetry search of a 3-D map (csrc/symmetry_search.inc): for every candidate (twist, rise, Csym)
 *     S = apply_helical_symmetry(V, apix, twist, rise, csym, fraction, new_size = V.shape, new_apix = apix)   (transforms.py:58-165)
 *     score = cross_correlation_coefficient(V[M], S[M])      Pearson; 0 where either side has no variance
 * over the region M = { (k, j, i) : rmin^2 <= (j - ny/2)^2 + (i - nx/2)^2 < rmax^2 and -h <= k - nz/2 < h } (integer
 * centres; h = max(1, int(nz z_fraction + 0.5) / 2), every plane when z_fraction >= 1).  An hh_hs keeps the map (host
 * float32 [shape[0]][shape[1]][shape[2]] = z, y, x, every side in [2, 1024]) on the device; a search uploads the list,
 * computes S on the voxels of M only without storing it, and returns one float32 score per candidate.  A score depends on
 * the candidate and the region alone: not on the list around it, nor on how the list is cut into launches.
 * hh_hs_create sets the default region rmin = 0, rmax = min(ny, nx) / 2 - 1, z_fraction = 0.5 (a map too small to have
 * one is created without and needs hh_hs_set_region).  Errors of a handle are read with hh_hs_last_error(handle), those of
 * hh_hs_create with hh_hs_last_error(NULL). */
typedef struct hh_hs hh_hs;
int hh_hs_create(hh_hs** out, int device, const float* map, const int32_t shape[3], double apix, double fraction);
/* rmax_px < 0: no outer limit.  A region without voxels is HH_ERR_ARG (and the handle is left without a region). */
int hh_hs_set_region(hh_hs* hs, double rmin_px, double rmax_px, double z_fraction);
/* Device bytes the per-workgroup partial sums of ONE launch may take (default 64 MiB, or the environment's
 * HELICON_HS_PARTIAL_BYTES when the handle is created): a list that needs more is cut into several launches of at
 * least one candidate each.  The scores do not depend on it. */
int hh_hs_set_budget(hh_hs* hs, int64_t partial_bytes);
/* params: [g][3] host float64 = twist (degrees), rise (Angstrom), csym; scores: [g] host float32.  rise <= 0 or not
 * finite, a twist that is not finite, or csym not a whole number in [1, 4096] is HH_ERR_ARG with the candidate's index in
 * the message; nothing is computed then. */
int hh_hs_search(hh_hs* hs, const double* params, int64_t g, float* scores);
/* z_range = the source planes [z0, z1) the operator reads (the 1 % profile rule and `fraction`), region_voxels = |M|,
 * launches = scoring launches since the handle was created; any of them may be NULL */
int hh_hs_info(const hh_hs* hs, int32_t z_range[2], int64_t* region_voxels, int64_t* launches);
/* device time of the last search's kernels (scoring + finalising, all launches), from events on the handle's stream */
int hh_hs_kernel_ms(const hh_hs* hs, double* ms);
void hh_hs_destroy(hh_hs* hs);
const char* hh_hs_last_error(const hh_hs* hs);

/* ---------------------------------------------------------------------------------------------
 * Fourier shell / ring correlation (csrc/fourier_correlation.inc; lib/analysis.py:116-356 calc_fsc, calc_fsc_per_shell,
 * calc_frc_2d).  `batch` pairs of equal size in one call (host float32, contiguous); per pair and shell the three sums
 *     num = sum w Re(F1 conj F2),   den1 = sum w |F1|^2,   den2 = sum w |F2|^2
 * come back as host float64 [batch][shells][3]; the ratio and its `denominator > 0` rule are the caller's.  float32
 * transforms, float64 products, sums that are bit-identical from run to run and do not depend on the batch.  Errors are
 * read with hh_last_error(NULL).  kernel_ms (may be NULL): device time of the kernels.
 * hh_fsc_3d: cubes of side n in [8, 512]; shells n / 2 + 1; shell = clip(round(sqrt(kz^2 + ky^2 + kx^2)), 0, n / 2) over
 * the half spectrum kx <= n / 2, every bin once (full_spectrum = 0: calc_fsc) or with the Hermitian weight, which equals
 * the sums over the full spectrum (full_spectrum = 1: calc_fsc_per_shell). */
int hh_fsc_3d(int device, const float* maps1, const float* maps2, int32_t batch, int32_t n, int full_spectrum, double* sums,
              double* kernel_ms);
/* images [ny][nx], both sides in [8, 1024], full spectrum; shell: host table [ny][nx] with entries in [0, n_shells]
 * (n_shells <= 512), sums: [batch][n_shells + 1][3] */
int hh_frc_2d(int device, const float* imgs1, const float* imgs2, int32_t batch, int32_t ny, int32_t nx, const int32_t* shell,
              int32_t n_shells, double* sums, double* kernel_ms);

/* ---------------------------------------------------------------------------------------------
 * Phase-randomised ("true") FSC of two half maps (csrc/true_fsc.inc; commands/trueFSC.py, lib/filters.py:469-520
 * randomize_phases_lowpass).  A context keeps one pair of cubic maps of EVEN side n in [8, 512] on the device, together with
 * their phase-randomised versions: every bin of the rfftn half spectrum with kz^2 + ky^2 + kx^2 >= m_cut (folded integer
 * frequencies) becomes |F| e^{i theta}, the bins below stay as they are; the maps come back through the inverse transform
 * with irfftn's semantics.  theta: phases1 / phases2 (host float64 [n][n][n / 2 + 1], radians; both or neither), or, when they
 * are NULL, a Philox4x32-10 draw with key = seed and counter = (bin index, map index).  Errors: hh_last_error(NULL). */
typedef struct hh_tfsc hh_tfsc;
int hh_tfsc_create(hh_tfsc** out, int device, const float* map1, const float* map2, int32_t n, int64_t m_cut,
                   const double* phases1, const double* phases2, uint64_t seed);
/* sums: [2][n / 2 + 1][3] num, den1, den2 of the unmasked curve and of the randomised-unmasked curve (every bin of the half
 * spectrum once, as calc_fsc counts them); the first equals hh_fsc_3d(full_spectrum = 0) bit for bit */
int hh_tfsc_curves(hh_tfsc* ctx, double* sums);
/* which = 0 / 1: the randomised map [n][n][n] (map_out, may be NULL) and / or its stored half spectrum, interleaved
 * complex64 [n][n][n / 2 + 1][2] (spec_out, may be NULL) */
int hh_tfsc_download(hh_tfsc* ctx, int which, float* map_out, float* spec_out);
/* masks1 (and masks2, or NULL: one mask for both members): host float32 [batch][n][n][n].  sums: [batch][2][n / 2 + 1][3] of
 * the pairs (map1 m1, map2 m2) and (map1r m1, map2r m2), with hh_fsc_3d's meaning of full_spectrum and its guarantees:
 * bit-identical from run to run, independent of the batch and of a mask's place in it.  Only the masks are uploaded. */
int hh_tfsc_masked(hh_tfsc* ctx, const float* masks1, const float* masks2, int32_t batch, int full_spectrum, double* sums,
                   double* kernel_ms);
int hh_tfsc_destroy(hh_tfsc* ctx);

/*
 * Soft masks of the true FSC built on the device (csrc/soft_mask.inc; commands/trueFSC.py:738-781 _soft_mask as
 * helicon_amd.true_fsc.soft_mask restates it).  support: uint8, nonzero = inside.  step = max(1, int(w / 4)); the support is
 * taken at every step-th voxel (m_a = ceil(n_a / step) samples per axis); D2 is the exact squared Euclidean distance, in
 * decimated voxels, to the nearest decimated inside voxel; step sqrt(D2) is interpolated back as scipy.ndimage.zoom(order=1,
 * mode="constant") does it (a coordinate beyond the last sample reads 0); on outside voxels the mask is
 * (cos(dist / w pi / 2) + 1) / 2 for 0 < dist <= w and 0 for dist > w, everywhere else 1.  A support without an inside voxel
 * at that step is an argument error; w <= 0 returns the support as 0 / 1; a NaN or infinite w is an argument error.
 * Results are bit-identical from run to run.  Errors: hh_last_error(NULL).
 */
/* sqdist_out: int32 [ceil(nz / stride)][ceil(ny / stride)][ceil(nx / stride)]; sides in [1, 1024] */
int hh_edt_3d(int device, const uint8_t* support, int32_t nz, int32_t ny, int32_t nx, int32_t stride, int32_t* sqdist_out,
              double* kernel_ms);
/* mask_out: float32 [nz][ny][nx] */
int hh_soft_mask_3d(int device, const uint8_t* support, int32_t nz, int32_t ny, int32_t nx, double soft_width, float* mask_out,
                    double* kernel_ms);
/* host only: the per-axis tables of zoom(order=1) the mask kernel reads, n outputs over m <= n samples; [n] each */
int hh_soft_mask_taps(int32_t n, int32_t m, int32_t* i0, int32_t* i1, double* w0, double* w1, int32_t* outside);
/* the supports [n][n][n] of a true-FSC context, uploaded once (support2 NULL: one support for both members) */
int hh_tfsm_set_support(hh_tfsc* ctx, const uint8_t* support1, const uint8_t* support2);
/* the mask hh_tfsm_soft_masked would use for member `which` (0 / 1) at this width, float32 [n][n][n] */
int hh_tfsm_soft_mask(hh_tfsc* ctx, int which, double soft_width, float* mask_out);
/* hh_tfsc_masked with the masks built on the device from the supports, one per width: nothing but the widths' tap tables is
 * uploaded.  sums: [batch][2][n / 2 + 1][3]; the same guarantees: bit-identical from run to run, independent of the batch and
 * of a width's place in it, and equal to hh_tfsc_masked of hh_tfsm_soft_mask's masks bit for bit. */
int hh_tfsm_soft_masked(hh_tfsc* ctx, const double* soft_widths, int32_t batch, int full_spectrum, double* sums,
                        double* kernel_ms);

/*
 * The adaptive mask of the true FSC built on the device (csrc/adaptive_mask.inc; commands/trueFSC.py:660-735
 * _generate_adaptive_mask as helicon_amd.true_fsc.adaptive_mask restates it): the volume in float64, low-passed by
 * scipy.ndimage.gaussian_filter's rule (sigma > 0; passes z, y, x, "reflect" boundary, unfused products and sums),
 * thresholded, and the 26-connected components of {LP > threshold} that hold a voxel >= v*, the 1000th largest value, kept
 * (all of them, if none holds one).  Every voxel tied at v* is a seed (np.argpartition keeps an arbitrary 1000).
 * taps: host float64 [int(4 sigma + 0.5) + 1], w[j] = exp(-0.5 / sigma^2 j^2) / sum as NumPy computes them
 * (helicon_amd.true_fsc.gaussian_taps): the library does not recompute them, so that the filter equals SciPy's bit for
 * bit; int(4 sigma + 0.5) <= 4096.  Sides in [1, 1024], at most 2^28 voxels; a mask needs at least 1000.  A NaN or infinite
 * voxel, and a constant volume in Otsu mode, are argument errors.  The labelling's loops are bounded: a defect returns
 * HH_ERR_INTERNAL.  Results are bit-identical from run to run.  Errors: hh_last_error(NULL).
 */
/* host only: np.linspace(hmin, hmax, 257) (edges_out [257], may be NULL) and Otsu's threshold from 256 counts */
int hh_am_otsu(const int64_t* counts, double hmin, double hmax, double* edges_out, double* threshold_out);
/* device-event milliseconds of the mask calls since the last reset, [8]: the z, y, x passes, statistics (minimum, maximum,
 * histogram, selection), runs, unions, flatten, pick; out may be NULL; reset != 0 zeroes them */
int hh_am_stage_ms(double* out, int reset);
/* vol, out: host float64 [nz][ny][nx] */
int hh_am_gaussian_3d(int device, const double* vol, int32_t nz, int32_t ny, int32_t nx, double sigma, const double* taps, double* out);
/* binary: host uint8, nonzero = foreground; roots_out: int32, the smallest flat index of the voxel's 26-connected component,
 * -1 on background */
int hh_am_label_3d(int device, const uint8_t* binary, int32_t nz, int32_t ny, int32_t nx, int32_t* roots_out, int64_t* n_components);
/* vol: host float64 (is_f64 != 0) or float32, widened exactly.  sigma = 0: no filter (taps may be NULL).  mode 0: Otsu;
 * 1: value x max(LP); 2: value; 3: the voxel at index `value` (a whole number) of LP sorted in descending order.
 * support_out: uint8 0 / 1.  info (may be NULL) [8]: threshold, min(LP), max(LP), v*, voxels above the threshold, voxels
 * kept, components, bits (1: no component held a seed and the mask is {LP > threshold}; 2: more than 1000 voxels >= v*) */
int hh_am_mask_3d(int device, const void* vol, int is_f64, int32_t nz, int32_t ny, int32_t nx, double sigma, const double* taps, int mode,
                  double value, uint8_t* support_out, double* info);
/* the support(s) of a true-FSC context from its resident float32 maps: of (double(map1) + double(map2)) / 2 for both members
 * (one_mask != 0), or one of each map; left where hh_tfsm_set_support leaves them.  info (may be NULL): [2][8] */
int hh_am_context_support(hh_tfsc* ctx, int one_mask, double sigma, const double* taps, int mode, double value, double* info);
/* the context's support for member `which` (0 / 1), uint8 [n][n][n] */
int hh_am_context_get_support(hh_tfsc* ctx, int which, uint8_t* support_out);

/*
 * Structure factors (csrc/structure_factor.inc; lib/filters.py:22-208 calculate_structural_factor, set_structural_factors,
 * match_structural_factors): the power |F|^2 of 3-D maps (nz, ny, nx; sides in [2, 512]) or 2-D images (ny, nx; sides in
 * [2, 1024]) summed over the full spectrum into the reference's bins, and the maps scaled so that their profile becomes a
 * target's.  Any sides, odd, prime and unequal included.  The binning tables are the host's, so that they are NumPy's own
 * values: qbins = np.linspace(0, nbins qstep, nbins) [nbins] (2 <= nbins <= 726, qbins[0] = 0, increasing), freq = the
 * np.fft.fftfreq tables of the axes, concatenated in the order of the shape.  A bin (kz, ky, kx) has the radius
 * qr = sqrt(qx^2 + qy^2 [+ qz^2]) / apix in float64, formed as NumPy forms it (ties are real), and the label
 * searchsorted(qbins, qr, "right") - 1; the last bin is open-ended.  target (may be NULL: a context for profiles only):
 * the target profile on qbins [nbins].  A context keeps the operators and a grow-only scratch; a batch is cut into chunks
 * of the scratch cap.  Errors: hh_last_error(NULL).
 */
typedef struct hh_sf hh_sf;
int hh_sf_create(hh_sf** out, int device, int32_t ndim, const int32_t* shape, double apix, int32_t nbins, const double* qbins,
                 const double* target, const double* freq);
/* maps: host float32 [batch][shape].  has_thresh != 0: clip(x, thresh, None) - thresh first; mask (may be NULL, [shape], one
 * for the batch): then x mask.  sums: float64 [batch][nbins], bit-identical from run to run and independent of the batch and
 * of a map's place in it; a map with a NaN gives NaN sums.  spec_out (may be NULL): the half spectrum of the prepared maps,
 * interleaved complex64 [batch][shape with nx / 2 + 1 for nx][2] */
int hh_sf_profile(hh_sf* ctx, const float* maps, int32_t batch, const float* mask, int has_thresh, double thresh, double* sums,
                  float* spec_out);
/* maps_out [batch][shape]: irfftn(F ratio_interp(qr)), ratio = sqrt(target / sums) per map (0 where sums == 0),
 * ratio_interp linear between the edges of qbins, ratio[nbins - 1] at qr == qbins[nbins - 1] and 0 above.  F is the spectrum
 * of the thresholded maps, or, when a mask is given, of the RAW maps (the profile still comes from the thresholded and masked
 * ones).  sums (may be NULL): the profile of every map, as hh_sf_profile returns it.  The same guarantees: bit-identical
 * from run to run and independent of the batch.  HH_ERR_STATE on a context without a target. */
int hh_sf_match(hh_sf* ctx, const float* maps, int32_t batch, const float* mask, int has_thresh, double thresh, float* maps_out,
                double* sums);
/* device-event milliseconds of the last call, [4]: the profile (prologue, forward passes, sums, ratio), the second transform
 * of a masked match, the scaling, the inverse passes */
int hh_sf_kernel_ms(hh_sf* ctx, double* ms);
int hh_sf_destroy(hh_sf* ctx);

/* ---------------------------------------------------------------------------------------------
 * Local resolution of two half maps (csrc/local_resolution.inc): the FSC of every window pair of even side w around a list of
 * centres, and the resolution at which each curve first falls below a threshold.  A window is lib/transforms.py:516-555
 * get_clip3d(map, c - w / 2, w) (zeros outside the map) times taper[z] taper[y] taper[x] (the 1-D profile of
 * lib/filters.py:415-466 generate_tapering_filter, built by the caller); its curve fsc[0 .. w / 2] is calc_fsc_per_shell's
 * (hh_fsc_3d with full_spectrum = 1, and 1.0 where the denominator is not positive); with saxis[k] = k / (w apix) and k* the
 * smallest k >= 1 with fsc[k] < threshold its resolution is 1 / saxis[w / 2] when there is no k*, w apix when k* = 1, else
 * 1 / (saxis[k* - 1] + (threshold - fsc[k* - 1]) (saxis[k*] - saxis[k* - 1]) / (fsc[k*] - fsc[k* - 1])).
 * A context keeps both maps [nz][ny][nx], sides in [8, 512], on the device.  Errors: hh_last_error(NULL). */
typedef struct hh_lres hh_lres;
int hh_lres_create(hh_lres** out, int device, const float* map1, const float* map2, int32_t nz, int32_t ny, int32_t nx);
int hh_lres_destroy(hh_lres* ctx);
/* window: even, in [8, 64]; taper: [window]; centres: [n][3] (z, y, x), inside the map; threshold in (-1, 1);
 * route: 0 automatic, 1 one workgroup per window pair with both half spectra in LDS (window <= 24), 2 gathered windows
 * through the passes of hh_fsc_3d (any window).  resolution: [n]; curves: [n][window / 2 + 1] or NULL; kernel_ms: device-event
 * milliseconds of the launches, or NULL.  A route's results are bit-identical from run to run and do not depend on the
 * budget or on the order of the centres.  HH_ERR_ARG: an odd or out-of-range window, a centre outside the map, a route
 * that cannot take the window, a threshold that is NaN or outside (-1, 1), a NULL. */
int hh_lres_run(hh_lres* ctx, int32_t window, const float* taper, const int32_t* centres, int64_t n, double apix, double threshold,
                int route, double* resolution, double* curves, double* kernel_ms);
/* caps of the later runs: device scratch of one chunk of the passes route, windows of one launch of either route
 * (0: the defaults) */
int hh_lres_set_budget(hh_lres* ctx, int64_t scratch_bytes, int64_t max_windows_per_launch);
/* host arithmetic only: the route a run would take (1 / 2), the LDS route's bytes per workgroup for this window (0 above 24)
 * and the windows of one launch under the budget; every output may be NULL.  HH_ERR_ARG as hh_lres_run. */
int hh_lres_plan(int32_t window, int route, int64_t scratch_bytes, int64_t max_windows_per_launch, int32_t* route_out,
                 int64_t* lds_bytes, int64_t* windows_per_launch);
/* grid: host float64 [gz][gy][gx], NaN = not evaluated, the value of centre step / 2 + i step along each axis; out: host
 * float32 [nz][ny][nx], trilinear between the centres: per axis u = clip((p - step / 2) / step, 0, g - 1),
 * i0 = min(floor(u), g - 2) (g == 1: that one corner), NaN corners dropped and the other weights renormalised, NaN where
 * the remaining weights sum to 0.  Map sides in [1, 512]. */
int hh_lres_upsample(int device, const double* grid, int32_t gz, int32_t gy, int32_t gx, int32_t step, int32_t nz, int32_t ny,
                     int32_t nx, float* out);

/* Batched 2-D image alignment (lib/alignment.py:8-239, align_images): one evaluation of the reference's objective — warp the
 * moving plane by xform.inverse (order 1, mode "constant"), integer shift by phase cross-correlation (skimage's
 * normalization = "phase", upsample_factor 1, no disambiguation), warp the plane and its taper again with that shift in mode
 * "wrap", Pearson coefficient of (reference, warped)[warped taper > 0] — for many candidates at once.  A context keeps the
 * prepared float32 reference plane [ny][nx] (and its half spectrum), n_moving prepared moving planes and their taper planes
 * (already padded to the reference's shape), each plane's range and the transform tables; sides in [2, 1024], odd or even.
 * inv_matrix: the first two rows of xform.inverse of the UNSHIFTED transform, float64, (x, y, 1) columns as scikit-image keeps
 * them.  shift_out: [n][2] (y, x); score_out: [n] (0 when the norm is 0, NaN on an empty mask); peak_out: [n] the maximum of
 * |c| (or NULL); nmask_out: [n] pixels under the warped taper (or NULL).  A result is bit-identical from run to run and does
 * not depend on the other candidates of the call or on its place among them.  Errors: hh_last_error(NULL). */
typedef struct hh_align hh_align;
int hh_align_chunk(void);   /* candidates of one launch group (compiled in) */
int hh_align_create(int device, int32_t ny, int32_t nx, const float* ref_work, int32_t n_moving, const float* moving_work,
                    const float* taper, hh_align** out);
int hh_align_destroy(hh_align* ctx);
int hh_align_eval(hh_align* ctx, int64_t n, const int32_t* moving_index, const double* inv_matrix, int32_t* shift_out,
                  double* score_out, float* peak_out, int32_t* nmask_out);
/* the correlation surface c [ny][nx] of one candidate (the arg-max of |c| is its shift) */
int hh_align_correlation(hh_align* ctx, int32_t moving_index, const double* inv_matrix, float* out);
/* the second warp (mode "wrap", the transform shifted by shift = (y, x)) of a resident plane (plane NULL; which: 0 the moving
 * plane, 1 its taper) or of the caller's plane [ny][nx] */
int hh_align_warp_wrap(hh_align* ctx, const float* plane, int32_t moving_index, int which, const double* inv_matrix,
                       const int32_t* shift, float* out);
/* phase_ms (or NULL): [5] device-event milliseconds of hh_align_eval since the last reset: warp, forward passes, inverse y
 * pass, c2r + arg-max, score.  enable: 1 / 0 switches the timing (each chunk is then synchronised) and resets, < 0 leaves it. */
int hh_align_profile(hh_align* ctx, int enable, double* phase_ms);

/* Type-2 non-uniform DFT of a stack of images at arbitrary points (plugins/images2star/calibratepixelsize.py:88-156): what
 * finufft.nufft2d2(x, y, f, eps = 1e-6) approximates, as the direct sum (isign = -1, centred modes, x with the FIRST axis)
 *     F[b][p] = sum_a sum_c images[b][a][c] exp(-i (x[p] (a - ny / 2) + y[p] (c - nx / 2)))      (integer halves)
 * images: host float32 [n_img][ny][nx], sides in [1, 16384]; x, y: host float64 [n_pts], radians per pixel, any real value
 * (phases are reduced in float64 before a sine is taken).  The columns are contracted on the f32 MFMA on images whose
 * float64 mean was removed; the mean's separable term is added in float64, so the result is the full sum.
 * mode 0: out = complex64 [n_img][n_pts] (re, im pairs); 1: out = float32 [n_img][n_pts], |F|; 2: out = float32 [group], the
 * ring maximum max over b and over p with p % group == r of |F| (1 <= group <= n_pts; no F is stored), equal bit for bit to
 * the maximum of mode 1's values.  Points and images are cut into launch groups of hh_nudft_chunk() (compiled in).  A value
 * is bit-identical from run to run and depends neither on the other points or images of the call nor on its place among
 * them.  HH_ERR_ARG: a NULL, n_img < 1, n_pts < 1, a side outside [1, 16384], another mode, a group outside [1, n_pts].
 * Errors: hh_last_error(NULL). */
int hh_nudft_chunk(void);
int hh_nudft2d2(int device, int32_t n_img, int32_t ny, int32_t nx, const float* images, int64_t n_pts, const double* x,
                const double* y, int mode, int32_t group, void* out);
/* device-event milliseconds of the calling thread's last hh_nudft2d2 (centring, axis sums and products; no copies) */
int hh_nudft_kernel_ms(double* ms);

#ifdef __cplusplus
}
#endif
#endif /* HELICON_HIP_H */
