// groth16_pair.hpp -- the pairing side of sylow_hip_groth16_verify_batch.  Compiled as the tail of plk_multi.hip: it reuses that unit's
// line tables (k_pair_lines, line_get), its sliced table lease (lease_table_slices: multi_plan.hpp's slice_jobs under
// sylow_hip_set_scratch_limit), miller_product_tree and k_final_exp_jobs.  Which route a batch takes: multi_plan.hpp, groth16_tables.
//
// Proof i passes iff  e(A_i, B_i) e(-alpha, beta) e(-vk_x_i, gamma) e(-C_i, delta) == 1  (the EVM form with every pair negated).
//   PER CALL:  the line table of gamma and delta -- k_pair_lines on the "point" P = (1, 1), i.e. the lines before their scaling by a G1
//              point, two slots of one job, 39 KB -- and the raw Miller value of e(-alpha, beta), one loop.
//   PER PROOF: vk_x_i (groth16.hip), the lines of B_i scaled by A_i (k_pair_lines, one slot: 19.5 KB in HBM, sliced under the scratch
//              limit exactly as sylow_hip_multi_pairing_batch slices), then k_groth16_miller: one shared squaring per step and three lines --
//              B_i's from the per-proof table, gamma's and delta's from the per-call table (the same address for every lane pair), scaled
//              by -vk_x_i and -C_i in registers -- times the per-call Miller value, then k_final_exp_jobs and its is-one flag.
// Against four literal pairs per proof this walks one G2 point per proof instead of four and runs three lines per step instead of four.
// Batches that multi_pairing_batch would send to its one-wavefront route (n <= 1024 and 4 n <= WIDE_MAX), and batches whose scratch limit
// is below 1024 proofs' tables, take the COMPOSED route: the four literal pairs per proof through sylow_hip_multi_pairing_batch.
namespace plk {
// the per-call operands: P = (1, 1) twice, Q = gamma, delta, offsets {0, 2}; -alpha and beta
__global__ void k_groth16_vk_setup(const u64* alpha, const u64* beta, const u64* gamma, const u64* delta, u64* ones, u64* gd, u64* off, u64* nalpha, u64* beta_out) {
  const int t = threadIdx.x;
  if (t < 16) {
    ones[t] = ((t >> 1) & 3) == 0 ? 1 : 0;              // [8][2]: word 0 of x and of y is 1
    gd[2 * t] = gamma[t]; gd[2 * t + 1] = delta[t];     // [16][2]
    beta_out[t] = beta[t];
  }
  if (t < 2) off[t] = 2 * (u64)t;
  if (t == 0) {
    store_fp(nalpha, 1, 0, 0, load_fp(alpha, 1, 0, 0));
    store_fp(nalpha, 1, 0, 4, fp_neg(load_fp(alpha, 1, 0, 4)));
  }
}
// the composed route's pair list: pairs 4 i .. 4 i + 3 of job i = (-A_i, B_i), (alpha, beta), (vk_x_i, gamma), (C_i, delta); off [n + 1]
__global__ void __launch_bounds__(BLOCK) k_groth16_pairs(const u64* alpha, const u64* beta, const u64* gamma, const u64* delta,
                                                         const u64* a, const uint8_t* ainf, const u64* b, const uint8_t* binf, const u64* c, const uint8_t* cinf,
                                                         const u64* vkx, const uint8_t* vkx_inf, size_t n, u64* pxy, uint8_t* pinf, u64* qxy, uint8_t* qinf, u64* off) {
  const size_t i = TID;
  if (i > n) return;
  off[i] = 4 * i;
  if (i == n) return;
  const size_t m = 4 * n, k = 4 * i;
  store_fp(pxy, m, k, 0, load_fp(a, n, i, 0)); store_fp(pxy, m, k, 4, fp_neg(load_fp(a, n, i, 4)));
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    pxy[(size_t)w * m + k + 1] = alpha[w];
    pxy[(size_t)w * m + k + 2] = vkx[(size_t)w * n + i];
    pxy[(size_t)w * m + k + 3] = c[(size_t)w * n + i];
  }
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    qxy[(size_t)w * m + k] = b[(size_t)w * n + i];
    qxy[(size_t)w * m + k + 1] = beta[w];
    qxy[(size_t)w * m + k + 2] = gamma[w];
    qxy[(size_t)w * m + k + 3] = delta[w];
  }
  pinf[k] = ainf && ainf[i]; pinf[k + 1] = 0; pinf[k + 2] = vkx_inf[i]; pinf[k + 3] = cinf && cinf[i];
  qinf[k] = binf && binf[i]; qinf[k + 1] = 0; qinf[k + 2] = 0; qinf[k + 3] = 0;
}
// PHASE B of the table route (see the head of this file).  table: k_pair_lines' layout with kt = 1 for the jb proofs of this slice;
// shared: the same layout with jb = 1, kt = 2 (slot 0 = gamma, slot 1 = delta), lines scaled by the isomorphism's constants only;
// fab: the per-call Miller value (48 words, stride 1).  An identity vk_x_i or a flagged C_i turns its line into the unit line (EIP-197).
__global__ void HEAVY_BOUNDS k_groth16_miller(const u32x4* table_generic, size_t jb, const u32x4* shared_generic, const u64* vkx, const uint8_t* vkx_inf,
                                              const u64* cxy, const uint8_t* cinf, size_t n, size_t job0, const u64* fab, u64* fout) {
  typedef const __attribute__((address_space(1))) u32x4* gptr;
  const size_t t = TID, jl = pair_index(t);
  const int odd = pair_role(t);
  const bool active = jl < jb;
  const size_t i = job0 + (active ? jl : 0);
  const bool live_x = !vkx_inf[i], live_c = !(cinf && cinf[i]);
  // the lines of gamma and delta are evaluated at -vk_x_i and -C_i: (l0, l1 (-y), l2 x)
  // the four scale factors live in LDS, not in 36 registers next to the accumulator and two lines
  __shared__ i32 coord[4][9][BLOCK];
  {
    const F29 xx = f29_reduce(f29_from_fp(load_fp(vkx, n, i, 0))), xy = f29_reduce(f29_from_fp(fp_neg(load_fp(vkx, n, i, 4))));
    const F29 cx = f29_reduce(f29_from_fp(load_fp(cxy, n, i, 0))), cy = f29_reduce(f29_from_fp(fp_neg(load_fp(cxy, n, i, 4))));
#pragma unroll
    for (int q = 0; q < 9; ++q) { coord[0][q][threadIdx.x] = xx.v[q]; coord[1][q][threadIdx.x] = xy.v[q]; coord[2][q][threadIdx.x] = cx.v[q]; coord[3][q][threadIdx.x] = cy.v[q]; }
  }
  auto coord_get = [&](int c) {                             // a lane reads back only what it wrote: no barrier
    F29 r;
#pragma unroll
    for (int q = 0; q < 9; ++q) r.v[q] = coord[c][q][threadIdx.x];
    return r;
  };
  const size_t stride = 2 * jb, line_step = (size_t)LT_CHUNKS * stride;
  const gptr at = (gptr)table_generic + 2 * (active ? jl : 0) + (size_t)odd;
  const gptr sh = (gptr)shared_generic + (size_t)odd;
  const W2 w_one = w2_from_s2(s2_one()), w_zero = W2{F29{{0, 0, 0, 0, 0, 0, 0, 0, 0}}};
  W12 f;
  {
    S12 one = s12_one();
    w12_from_s12(f, one);
  }
  const u64 nz = BN_ATE_NAF_NZ;
  int line = 0;
  auto lines = [&]() {
    const gptr srow = sh + (size_t)line * (2 * LT_CHUNKS * 2);
    {
      const LineW L = line_get(at + (size_t)line * line_step, stride);
      const LineW G = line_get(srow, 2);
      const W12 ll = w12_line_product(L.l0, L.l4, L.l2, w2_select(w_one, G.l0, live_x), w2_select(w_zero, w2_scale(G.l4, coord_get(1)), live_x),
                                      w2_select(w_zero, w2_scale(G.l2, coord_get(0)), live_x));
      f = w12_mul_line_pair(f, ll);
    }
    {
      const LineW D = line_get(srow + LT_CHUNKS * 2, 2);
      f = w12_sparse_mul(f, w2_select(w_one, D.l0, live_c), w2_select(w_zero, w2_scale(D.l4, coord_get(3)), live_c), w2_select(w_zero, w2_scale(D.l2, coord_get(2)), live_c));
    }
    ++line;
  };
#pragma unroll 1
  for (int it = 0; it < 64; ++it) {
    f = w12_sqr(f);
    lines();
    if ((nz >> (63 - it)) & 1) lines();
  }
  lines();
  lines();
  W12 rest;
  {
    S12 fs;
    load_s12(fs, fab, 1, 0, odd);
    w12_from_s12(rest, fs);
  }
  f = w12_mul(f, rest);                                 // by value: the accumulator never leaves the registers
  S12 fin;
  w12_to_s12(fin, f);
  if (active) store_s12(fout, jb, jl, odd, fin);
}
}  // namespace plk

// the composed route: four literal pairs per proof through sylow_hip_multi_pairing_batch (whatever route that takes at this size)
static int32_t groth16_verify_composed(const uint64_t* vk_alpha, const uint64_t* vk_beta, const uint64_t* vk_gamma, const uint64_t* vk_delta,
                                       const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy, const uint8_t* c_inf,
                                       const uint64_t* vkx, const uint8_t* vkx_inf, size_t n, uint8_t* ok, void* stream) {
  const size_t m = 4 * n;
  host::Lease ws;
  int32_t rc = ws.acquire((24 * m + n + 1) * sizeof(u64) + 2 * m, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *pxy = (u64*)ws.p, *qxy = pxy + 8 * m, *off = qxy + 16 * m;
  uint8_t *pinf = (uint8_t*)(off + n + 1), *qinf = pinf + m;
  plk::k_groth16_pairs<<<GRID(n + 1)>>>(vk_alpha, vk_beta, vk_gamma, vk_delta, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, vkx, vkx_inf, n, pxy, pinf, qxy, qinf, off);
  rc = sylow_hip_multi_pairing_batch(pxy, pinf, qxy, qinf, off, n, m, /*skip_infinity=*/1, nullptr, ok, stream);
  return host::finish(rc, ws);
}

extern "C" int32_t sylow_hip_groth16_verify_batch(const uint64_t* vk_alpha, const uint64_t* vk_beta, const uint64_t* vk_gamma, const uint64_t* vk_delta,
                                                  const uint64_t* vk_ic, size_t n_inputs, const uint64_t* a_xy, const uint8_t* a_inf,
                                                  const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy, const uint8_t* c_inf,
                                                  const uint64_t* inputs, size_t n, uint8_t* ok, void* stream) {
  ARGCHK(ok && (n == 0 || (vk_alpha && vk_beta && vk_gamma && vk_delta && vk_ic && a_xy && b_xy && c_xy && (inputs || !n_inputs)))); if (!n) return SYLOW_HIP_OK;
  hipStream_t st = (hipStream_t)stream;
  host::Lease wx;                                              // vk_x [8][n] + flags
  int32_t rc = wx.acquire(8 * n * sizeof(u64) + n, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64* vkx = (u64*)wx.p;
  uint8_t* vkx_inf = (uint8_t*)(vkx + 8 * n);
  rc = sylow_hip_groth16_vk_x_batch(vk_ic, n_inputs, inputs, n, vkx, vkx_inf, stream);
  if (rc != SYLOW_HIP_OK) return host::finish(rc, wx);
  const mp::Knobs knobs = knobs_now();
  if (!mp::groth16_tables(knobs, n)) {
    rc = groth16_verify_composed(vk_alpha, vk_beta, vk_gamma, vk_delta, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, vkx, vkx_inf, n, ok, stream);
    return host::finish(rc, wx);
  }
  // per call: operands, the gamma / delta line table, e(-alpha, beta)
  constexpr size_t SHARED_BYTES = mp::table_bytes_per_job(2);       // one job of two slots: gamma, delta
  host::Lease wv, wab, ws;
  rc = wv.acquire(SHARED_BYTES + (16 + 32 + 2 + 8 + 16) * sizeof(u64), st);
  if (rc != SYLOW_HIP_OK) return host::finish(rc, wx);
  plk::u32x4* shared = (plk::u32x4*)wv.p;
  u64 *ones = (u64*)((uint8_t*)wv.p + SHARED_BYTES), *gd = ones + 16, *off2 = gd + 32, *nalpha = off2 + 2, *beta = nalpha + 8;
  plk::k_groth16_vk_setup<<<1, 64, 0, st>>>(vk_alpha, vk_beta, vk_gamma, vk_delta, ones, gd, off2, nalpha, beta);
  plk::k_pair_lines<true><<<1, 64, 0, st>>>(ones, nullptr, gd, nullptr, off2, 0, 1, 2, 2, 1, shared);
  const u64* fab = nullptr;
  rc = miller_product_tree(knobs, nalpha, nullptr, beta, nullptr, 1, 1, wab, &fab, stream);
  if (rc != SYLOW_HIP_OK) return host::finish(rc, wab, wv, wx);
  // per proof, in slices under the table budget: one slot per job, and per slice its raw values; the proofs' offsets once
  const size_t per_job = mp::table_bytes_per_job(1), w_off = ((n + 2) & ~(size_t)1) * sizeof(u64);
  size_t jb_max = 0;
  rc = lease_table_slices(ws, knobs.budget, per_job, n, [&](size_t jb) { return 48 * jb * sizeof(u64) + w_off; }, st, &jb_max);
  if (rc != SYLOW_HIP_OK) return host::finish(rc, wab, wv, wx);
  plk::u32x4* table = (plk::u32x4*)ws.p;
  u64 *raw = (u64*)((uint8_t*)ws.p + per_job * jb_max), *off = raw + 48 * jb_max;
  plk::k_chunk_offsets<<<GRID(n + 1)>>>(off, n, n, 1, nullptr);
  for (size_t job0 = 0; job0 < n; job0 += jb_max) {
    const size_t jb = n - job0 < jb_max ? n - job0 : jb_max;
    plk::k_pair_lines<true><<<GRID(2 * jb)>>>(a_xy, a_inf, b_xy, b_inf, off, job0, jb, n, 1, 1, table);
    plk::k_groth16_miller<<<GRID(2 * jb)>>>(table, jb, shared, vkx, vkx_inf, c_xy, c_inf, n, job0, fab, raw);
    plk::k_final_exp_jobs<<<GRID(2 * jb)>>>(raw, jb, job0, jb, n, nullptr, ok);
  }
  return host::finish(SYLOW_HIP_OK, ws, wab, wv, wx);
}
