// cassie_pg_vjp_row.inc -- the row store of the width-128 VJP's workgroup, included behind the group loop of pg_vjp_kernel (tu_pg.hip) and
// w128::clip_grad_kernel (tu_ppo.hip); shared as text for the reason cassie_pg_vjp.inc gives (as a function it changes the instructions of both).
// The includer provides S = Shape<D, A>, float* out (the workgroup's row: [gW1 | gb1 | gW2 | gb2 | gW3 | gb3], NP floats; the row may be longer)
// and the accumulators of cassie_pg_vjp.inc.  gW[row_of(v, h)][c] in register v: wavefront q writes rows 32 q .. 32 q + 31 of gW1 / gb1 / gW2 / gb2
// and columns 32 q .. 32 q + 31 of gW3; wavefront 0 writes gb3.
  const int q = wave;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = row_of(v, h);
#pragma unroll
    for (int kb = 0; kb < NB; kb++) out[S::O_W2 + (32 * q + r) * H + 32 * kb + c] = gW2[kb][v];
    if (c < D) out[S::O_W1 + (32 * q + r) * D + c] = gW1[v];
    if (c == D) out[S::O_B1 + 32 * q + r] = gW1[v];
    if (r < A) out[S::O_W3 + r * H + 32 * q + c] = gW3[v];
  }
  gb2 += __shfl_xor(gb2, 32, 64); gb3 += __shfl_xor(gb3, 32, 64);
  if (h == 0) out[S::O_B2 + 32 * q + c] = gb2;
  if (q == 0 && h == 0 && c < A) out[S::O_B3 + c] = gb3;
