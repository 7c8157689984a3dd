// cassie_pg_vjp.inc -- the reverse pass of one group of four tiles of the width-128 VJP, from the cotangent to the three accumulations:
// the text pg_vjp_kernel (tu_pg.hip) and w128::clip_grad_kernel (tu_ppo.hip) share, included inside their group loop.
//
// Shared as TEXT, not as a function: both kernels sit at the register limit (256 VGPRs + 228 .. 248 AGPRs, no scratch).  As a __forceinline__ template
// (fragments as lambdas, accumulators by reference) the pass spilled 115 .. 131 registers to 464 .. 528 B of scratch per lane; two causes were found
// and both are avoided here: the row rule behind a function call in the index expressions (hence ROW_AT, cassie_tiles.h), and any new function
// or lambda in the unit, which changes the order the compiler inlines in and with it the instructions of EVERY kernel of the unit.  The included
// text with statement macros compiles to the instructions the kernels had with the pass written out twice (profiles/onpolicy_dedup_kernel_resources.txt).
//
// The includer provides, in scope:
//   D, A, c, h, wave                                the kernel's template parameters and lane / wavefront indices
//   Net th; v16f h1[NB], h2[NB], g2[NB], g1[NB]     this wavefront's tile: weights, activations of the forward pass, room for G2 and G1
//   float wt[4]                                     the tile's cotangent on the mean, row a = v + 4 h in wt[v]
//   float stage[2][WAVES][H * TP]                   the two LDS slots
//   v16f gW1, gW2[NB], gW3; float gb2, gb3          the workgroup's accumulators (wavefront q = wave: quarter q)
// and its two fragments as macros (a lambda is one more function for the inliner, and that alone changes the register allocation of every kernel
// of the unit), for tile u of the group; k-step e is sample 16 h + e of that tile:
//   PG_VJP_COT_ROW(u, wa)   fills float wa[16], the cotangent transposed: row (action) c at the 16 k-steps; zero for c >= A and past the end
//   PG_VJP_OBS_T(u, e, x)   x = [obs | 1] transposed: feature c at k-step e (0 past the end), 1 for c == D, 0 for c > D

    // G2 = (W3' w) o (1 - H2^2): k-step v sums over the cotangent row a = v + 4 h
#pragma unroll
    for (int ob = 0; ob < NB; ob++) {
      v16f y = zero16();
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int a = v + 4 * h;
        y = TILE_MFMA(a < A ? th.W3[a * H + 32 * ob + c] : 0.0f, wt[v], y);
      }
#pragma unroll
      for (int v = 0; v < 16; v++) y[v] *= 1.0f - h2[ob][v] * h2[ob][v];
      g2[ob] = y;
    }
    // Three exchanges through the two LDS slots, so that no more than two 128 x 32 activations of the tile are live in registers:
    // ---- 1. H1 (slot 0, kept to the third exchange) and H2 (slot 1): gW3[a][32 q + j] += sum_s w[s][a] H2[32 q + j][s]
    wave_put(stage[0][wave], h1, c, h);
    wave_put(stage[1][wave], h2, c, h);
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < WAVES; u++) {
      float ta[16], wa[16];
      PG_VJP_COT_ROW(u, wa);
      wave_get(stage[1][u] + 32 * wave * TP, ta, c, h);
#pragma unroll
      for (int s = 0; s < 16; s++) { gW3 = TILE_MFMA(wa[s], ta[s], gW3); gb3 += wa[s]; }
    }
    // ---- 2. G2 (slot 1): gW2[32 q + i][32 kb + j] += sum_s G2[32 q + i][s] H1[32 kb + j][s]
    __syncthreads();
    wave_put(stage[1][wave], g2, c, h);
    __syncthreads();
    // G1 = (W2' G2) o (1 - H1^2) of this wavefront's tile (H1 from its slot-0 image): k-step v of block (ob, kb) reads W2[32 kb + r(v, h)][32 ob + c]
    const float* myh1 = stage[0][wave];
#pragma unroll
    for (int ob = 0; ob < NB; ob++) {
      v16f y = zero16();
#pragma unroll
      for (int kb = 0; kb < NB; kb++)
#pragma unroll
        for (int v = 0; v < 16; v++) y = TILE_MFMA(th.W2[(size_t)ROW_AT(32 * kb, v, h) * H + 32 * ob + c], g2[kb][v], y);
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const float x = myh1[ROW_AT(32 * ob, v, h) * TP + c];
        y[v] *= 1.0f - x * x;
      }
      g1[ob] = y;
    }
#pragma unroll 1
    for (int u = 0; u < WAVES; u++) {
      float ta[16], tb[16];
      wave_get(stage[1][u] + 32 * wave * TP, ta, c, h);
#pragma unroll
      for (int s = 0; s < 16; s++) gb2 += ta[s];
#pragma unroll
      for (int kb = 0; kb < NB; kb++) {
        wave_get(stage[0][u] + 32 * kb * TP, tb, c, h);
#pragma unroll
        for (int s = 0; s < 16; s++) gW2[kb] = TILE_MFMA(ta[s], tb[s], gW2[kb]);
      }
    }
    // ---- 3. G1 (slot 0): gW1[32 q + i][k] += sum_s G1[32 q + i][s] [obs | 1][s][k]   (column D: gb1)
    __syncthreads();
    wave_put(stage[0][wave], g1, c, h);
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < WAVES; u++) {
      float ta[16], xt[16];
#pragma unroll
      for (int e = 0; e < 16; e++) PG_VJP_OBS_T(u, e, xt[e]);
      wave_get(stage[0][u] + 32 * wave * TP, ta, c, h);
#pragma unroll
      for (int s = 0; s < 16; s++) gW1 = TILE_MFMA(ta[s], xt[s], gW1);
    }
