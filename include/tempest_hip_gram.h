/*
 * tempest_hip_gram.h -- the Gram matrix of a buffer's frames, on the GPU.  Part of the C ABI of libtempest_hip.so: tempest_hip.h
 * includes this file once, after tempest_hip_ctrack.h; include tempest_hip.h, not this file.
 *
 * tempest_hip_cfold.h finds the carrier's advance kappa by folding the buffer once per trial; tempest_hip_ctrack.h measures a frame's
 * phase against a picture that something else has to supply.  Both rest on one quantity: G[f][g] = sum_m v_f(m) conj(v_g(m)), the
 * inner product of every pair of frames.  It is F x F complex numbers, each with the processing gain of all P pixels, and from it
 * alone the host has the energy of the coherent fold for ANY per-frame phases ((1/F^2) sum_fg w_f conj(w_g) G[f][g]: the whole kappa
 * periodogram from one pass, gram_carrier of the bindings) and every frame's phase against the stack of all the others with no
 * reference picture and no model of the drift (the leading eigenvector of G without its diagonal, gram_phases of the bindings).
 * The entry points below go beyond the reference and change nothing that exists.
 *
 *  1. INPUT, TRACK, SAMPLING.  Exactly tempest_hip_ctrack.h, 1. - 3.: iq, n, the format rule, the geometry y_t x x_t with P = y_t*x_t,
 *     t0, T, F = n_frames, z[k], amax; the track's (a_f, b_f) and the weight w_f(l) of frame f on line l; the sampled z_f(m) of pixel
 *     m = l*x_t + p.  As tempest_hip_ctrack.h, 8.:
 *       v_f(m) = w_f(l) * z_f(m)           in f32: re = fsub(fmul(wr, zr), fmul(wi, zi)), im = fadd(fmul(wr, zi), fmul(wi, zr))
 *     the probe's four products.  track may be NULL: the zero track, the same arithmetic on a = b = 0 (the bits of an all-zero
 *     track).  iq and the track are never written.
 *  2. RESULT.  gram holds 2*F*F doubles, row-major: gram[2*(f*F + g)] = Re G[f][g], gram[2*(f*F + g) + 1] = Im G[f][g],
 *       G[f][g] = sum_m v_f(m) conj(v_g(m)):   Re = sum vr_f vr_g + vi_f vi_g,   Im = sum vi_f vr_g - vr_f vi_g
 *     Both triangles are written: the entries with f >= g are computed, G[g][f] has the bits of conj(G[f][g]) (the same real part,
 *     the imaginary part with its sign flipped), and Im G[f][f] is +0.  G[f][f] is the probe's E_f (within the two bounds).
 *  3. SUMMATION.  A tile is 64 raster lines x 128 pixels of a line (64 x 16 when a line's span is too long: COST), the fold's tiles
 *     in the fold's order.  A tile's pixels are taken in CHUNKS of at most TSDR_GRAM_CHUNK = 1024 pixels (8 lines x 128, or 64 x 16).
 *     Inside a chunk the four real sums sum vr_f vr_g, sum vi_f vi_g, sum vi_f vr_g and sum vi_g vr_f run in f32, each
 *     product entering its sum through one fused multiply-add -- one rounding per term, no wider intermediate -- in a fixed pixel
 *     order: the f32-input matrix instruction of gfx950 (v_mfma_f32_32x32x2_f32), which is bit for bit an fmaf chain.  A chain holds
 *     at most 2 * TSDR_GRAM_CHUNK products (the two sums of Re may share one chain).  At the end of a chunk each chain is widened to
 *     f64 and added to the tile's f64 partial sum: chunks within a tile in chunk order; then, one lane per entry with f >= g,
 *     Re = the two partial sums of Re added, Im = the difference of the two partial sums of Im, per tile, and the tiles in tile order.
 *     No float atomics.
 *  4. ACCURACY.  The contract is an error bound, not a bit pattern.  u = 2^-24; eps_t = sqrt(2) * 12 * u * amax is the error of a
 *     term v_f(m) (tempest_hip_ctrack.h, 9.); E_f = G[f][f] of the reference; ref: the formulas in exact arithmetic on the same z
 *     and the same doubles of the track.  With v = ref + d, |d| <= eps_t:  v_f conj(v_g) - ref = d_f conj(ref_g) + ref_f conj(d_g) +
 *     d_f conj(d_g), summed over P pixels with Cauchy-Schwarz:   eps_t * (sqrt(P * E_f) + sqrt(P * E_g)) + P * eps_t^2.
 *     An fmaf chain of n products errs by at most n u sum |a b| (to first order); per pixel |vr_f vr_g| + |vi_f vi_g| <= |v_f| |v_g| and
 *     |vi_f vr_g| + |vr_f vi_g| <= |v_f| |v_g|, the sums of |v_f| |v_g| over a chunk and then over the chunks are at most sqrt(E_f * E_g)
 *     (Cauchy-Schwarz twice): Re within 2 * TSDR_GRAM_CHUNK u sqrt(E_f * E_g), Im within TSDR_GRAM_CHUNK u sqrt(E_f * E_g); with 64 u for
 *     the second order (n u against n u / (1 - n u), the computed terms against the exact ones):
 *       c = 3 * TSDR_GRAM_CHUNK + 64 = 3136,   the f32 chain term c * u * sqrt(E_f * E_g)
 *     The f64 sums are at most 8 chunks and
 *     fewer than TSDR_GRAM_MAX_TILES = 2^16 tiles deep (REFUSALS): 2^-36 * sqrt(E_f * E_g).  Together
 *       |G[f][g] - ref| <= eps_t * (sqrt(P * E_f) + sqrt(P * E_g)) + P * eps_t^2 + (c * u + 2^-36) * sqrt(E_f * E_g)
 *     (the chain term is a worst case, linear in the chain's length; the errors observed are near its square root: the GPU tests
 *     print the worst ratio).
 *  5. REPRODUCIBILITY, FORMAT INVARIANCE.  Two calls with the same arguments leave identical bits in gram; the integer formats (sc16,
 *     sc8, uc8) give the bits of the host-expanded ComplexF32 buffer; the host form has the bits of the device form.
 *  6. REFUSALS.  TSDR_EINVAL, with nothing written and nothing enqueued, for everything tempest_hip_ctrack.h, 11. refuses of a fold's
 *     geometry (a NULL ctx or iq; an unknown format; y_t <= 0, x_t <= 0, P >= 2^31; n < 2 or n >= 2^31; F < 0; T or t0 not finite;
 *     T < 2; t0 < 0; t0 + F*T > n; iq not aligned), and for: gram NULL; n_frames > TSDR_GRAM_MAX_FRAMES;
 *     TSDR_GRAM_MAX_TILES tiles or more (SUMMATION: ceil(y_t / 64) * ceil(x_t / 128), or ceil(y_t / 64) * ceil(x_t / 16) when a line's
 *     span is too long); in the device form
 *     gram or a non-NULL track not 8-byte aligned; in the host form a track entry that is not finite.
 *     F == 0 is TSDR_OK and touches nothing.  Nothing is written outside gram[0 .. 2*F*F).
 *  7. COST.  "gram_tile" / "gram_direct" have the coherent fold's tiles and its tiled / direct choice (TSDR_CFOLD_STAGE_MAX), four
 *     wavefronts per workgroup.  A workgroup evaluates its tile's weights once (64 lines x F, as the tracked stack does per frame) and
 *     walks the tile in panels of 128 pixels: every lane samples and turns one pixel of the panel for half of the frames -- in the
 *     tiled kernel a wavefront's lanes are neighbours along a raster line, so their loads coalesce without staging -- and stores Re
 *     and Im into an LDS panel X[row][pixel], rows = the frames' real parts, then their imaginary parts, each padded with zeros to
 *     32 or 64.  After a barrier the wavefronts run the matrix instruction over the panel: with 32-row blocks R_i, I_i,
 *     Re G = R R^T + I I^T and Im G = I R^T - (I R^T)^T; the block products of one triangle -- 3 for F <= 32, 10 for F <= 64 -- are
 *     dealt to the wavefronts, so there is no reduction across wavefronts.  The accumulators are widened once per chunk.  LDS: 48.5 KiB
 *     at F <= 32, up to 97 KiB at F <= 64.  The workspace holds 24 KiB (F <= 32) or 56 KiB of f64 partial sums per tile; "gram_sum" adds the
 *     tiles, one lane per entry, and writes both triangles.  Measured on one MI355X (profiles/gram.json; 30 frames, ComplexF32): C2
 *     (2576x1125) 755 us beside the coherent fold's 130 us (5.8x) and the 120-trial carrier scan's 5698 us; C5 (4400x2250)
 *     1672 us beside 301 us (5.5x) and 19171 us.  Where the time goes: DESIGN.md section 4.
 * The `_d` form takes device pointers, enqueues on the context's stream and returns.  The host-pointer form uploads iq and the track,
 * runs the device form and copies gram back; its wait is bounded like every other host form's (option "wait_ms").
 */
#ifndef TEMPEST_HIP_GRAM_H
#define TEMPEST_HIP_GRAM_H
#ifndef TEMPEST_HIP_CTRACK_H
#error "include tempest_hip.h, which includes tempest_hip_gram.h after tempest_hip_ctrack.h"
#endif
#define TSDR_GRAM_MAX_FRAMES 64
#define TSDR_GRAM_CHUNK 1024
#define TSDR_GRAM_MAX_TILES 65536
/* gram[2*(f*F + g)], gram[2*(f*F + g) + 1] = Re, Im of sum_m v_f(m) conj(v_g(m)), the frames of `iq` turned along `track` (may be
 * NULL: the zero track), F = n_frames <= TSDR_GRAM_MAX_FRAMES (1. - 7. above), device pointers */
int tsdr_ctrack_gram_iq_d(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track,
                          int n_frames, int y_t, int x_t, double *gram);
/* the same with host pointers: upload, run, download gram */
int tsdr_ctrack_gram_iq(tsdr_ctx *ctx, const void *iq, int iq_fmt, float scale, size_t n, double t0, double T, const double *track,
                        int n_frames, int y_t, int x_t, double *gram);
#endif /* TEMPEST_HIP_GRAM_H */
