// Device probe of the randomized batch's scalar side -- TEST INFRASTRUCTURE.
//
// A sub-batch that fails bls381_verify_batch_randomized is re-verified item by item, so a wrong
// weight, R1 = [r_i] pk_i or S_b = sum_i [r_i] sig_i costs speed and never a verdict: the verdicts
// cannot show it.  This translation unit includes bls381_kernels.hpp and launches the product's own
// kernels, unchanged and with run_verify_randomized's workgroup and grid shapes, and hands every
// intermediate back to tests/test_randomized_scalars.py, which compares them with Python integers
// (tests/rb_model.py).  hipcc builds it into lib/libbls381_rbcheck.so.  The library is loaded only
// by tests; the product library (libbls381.so) never links it and it exports no bls381_* symbol.
//
// Launched, in the product's order: k_prologue_1<1> (dummy all-zero 32-byte messages and domains:
// the hash role's output is not read), k_rb_g2_test, then both routes to the sub-batch sums --
// k_rb_msm_sort / _bucket / _window / _combine (the product's route up to 256 items per
// sub-batch) and k_rb_scale_g2 (its per-item ladder above that).
//
// Boundary, as dev_check.hip: host pointers in and out, null stream, nothing left allocated,
// n <= 4096; every Fp crosses raw, as 14 little-endian u32 limb words (28-bit limbs) in the
// Montgomery domain (R = 2^392), nothing converted.  An Fp2 is (c0, c1); a G1 affine point 2 Fp;
// a G2 Jacobian point 3 Fp2 = 6 Fp.  One entry:
//   rbc_run(n, B, seed32, pks48, sigs96, strict, st, r1, r2, off, idx, bucket, win, sb)
//     st     [4][n]                 pk_st, sig_st, cls, r1_st of every item
//     r1     [n][2][14]             R1 affine (written where r1_st is ST_OK, else zeros)
//     r2     [n][6][14]             R2 Jacobian: k_rb_scale_g2's ladder
//     off    [nb][W][D + 1]         k_rb_msm_sort's list starts, nb = ceil(n / B)
//     idx    [nb][W][2 B]           its point numbers (u16; entries past off[D] are zeros)
//     bucket [nb][W][D][6][14]      k_rb_msm_bucket (digit-0 slots are zeros: never written)
//     win    [nb][W][6][14]         k_rb_msm_window
//     sb     [nb][6][14]            k_rb_msm_combine: S_b Jacobian
//   strict != 0: BLS381_POLICY_STRICT's flags, else BLS381_POLICY_PYECC's (bls381_capi.hip
//   policy_flags / check_subgroups).  Returns 0 or the HIP error code.
// rbc_dims(out[3]) = {RB_MSM_C, RB_MSM_W, RB_MSM_D}.
#include <cstring>
#include <vector>

#include "bls381.h"   // declarations only (the status codes bls381_kernels.hpp names): nothing here defines them
#include "bls381_kernels.hpp"

using namespace bls381;

namespace {

constexpr size_t MAX_N = 4096;
constexpr size_t MAX_B = 256;   // the product's RB_MSM_MAX_B

unsigned grid_for(size_t n) { return (unsigned)((n + KBLOCK - 1) / KBLOCK); }

// a zeroed device buffer, freed on scope exit
template <class T>
struct dev_buf {
  T* p = nullptr;
  size_t count;
  hipError_t err;
  explicit dev_buf(size_t c) : count(c ? c : 1) {
    err = hipMalloc((void**)&p, count * sizeof(T));
    if (err == hipSuccess) err = hipMemset(p, 0, count * sizeof(T));
  }
  ~dev_buf() { if (p) (void)hipFree(p); }
  dev_buf(const dev_buf&) = delete;
  dev_buf& operator=(const dev_buf&) = delete;
  hipError_t up(const void* src, size_t bytes) { return hipMemcpy(p, src, bytes, hipMemcpyHostToDevice); }
  hipError_t down(std::vector<T>& h) {
    h.resize(count);
    return hipMemcpy(h.data(), p, count * sizeof(T), hipMemcpyDeviceToHost);
  }
};

// SoA -> item-major.  One-lane items: limb k of Fp c of item i at src[(c 14 + k) cnt + i];
// lane-pair items: limb k of Fp2 component c, coefficient p, at src[(c 14 + k) 2 cnt + 2 i + p]
void unsoa_lane(uint32_t* dst, const std::vector<uint32_t>& src, size_t cnt, int nfp) {
  for (size_t i = 0; i < cnt; ++i)
    for (int c = 0; c < nfp; ++c)
      for (int k = 0; k < FP_LIMBS; ++k) dst[(i * nfp + c) * FP_LIMBS + k] = src[(size_t)(c * FP_LIMBS + k) * cnt + i];
}
void unsoa_pair(uint32_t* dst, const std::vector<uint32_t>& src, size_t cnt, int nfp2) {
  for (size_t i = 0; i < cnt; ++i)
    for (int c = 0; c < nfp2; ++c)
      for (int p = 0; p < 2; ++p)
        for (int k = 0; k < FP_LIMBS; ++k)
          dst[((i * nfp2 + c) * 2 + p) * FP_LIMBS + k] = src[(size_t)(c * FP_LIMBS + k) * 2 * cnt + 2 * i + p];
}

}  // namespace

extern "C" {

void rbc_dims(int out[3]) { out[0] = RB_MSM_C; out[1] = RB_MSM_W; out[2] = RB_MSM_D; }

int rbc_run(size_t n, size_t B, const uint8_t* seed32, const uint8_t* pks48, const uint8_t* sigs96, int strict,
            uint8_t* st, uint32_t* r1, uint32_t* r2, uint32_t* off, uint16_t* idx, uint32_t* bucket, uint32_t* win,
            uint32_t* sb) {
  if (n == 0 || n > MAX_N || B < 2 || B % 2 || B > MAX_B) return (int)hipErrorInvalidValue;
  if (!seed32 || !pks48 || !sigs96 || !st || !r1 || !r2 || !off || !idx || !bucket || !win || !sb)
    return (int)hipErrorInvalidValue;
  const size_t nb = (n + B - 1) / B;
  // the policy flags of run_verify_randomized: the key under the call's codec and subgroup mode,
  // the signature codec-only (its G2 test is k_rb_g2_test's)
  const int chk = strict ? 1 : 0, lax = strict ? 0 : CHK_LAX;
  const int pk_flags = chk | lax, sig_flags = lax;

  dev_buf<uint8_t> d_pks(48 * n), d_sigs(96 * n), d_msgs(32 * n), d_doms(8 * n), d_seed(64);
  dev_buf<uint32_t> pk_aff(2 * FP_LIMBS * n), sig_aff(4 * FP_LIMBS * n), h_aff(4 * FP_LIMBS * n);
  dev_buf<uint32_t> d_r1(2 * FP_LIMBS * n), d_r2(6 * FP_LIMBS * n);
  dev_buf<uint8_t> pk_st(n), sig_st(n), cls(n), r1_st(n);
  dev_buf<uint32_t> moff(nb * RB_MSM_W * (RB_MSM_D + 1));
  dev_buf<uint16_t> midx(nb * RB_MSM_W * 2 * B);
  dev_buf<uint32_t> mbucket(6 * FP_LIMBS * nb * RB_MSM_W * RB_MSM_D), mwin(6 * FP_LIMBS * nb * RB_MSM_W);
  dev_buf<uint32_t> mjac(6 * FP_LIMBS * nb);
  for (hipError_t e : {d_pks.err, d_sigs.err, d_msgs.err, d_doms.err, d_seed.err, pk_aff.err, sig_aff.err, h_aff.err,
                       d_r1.err, d_r2.err, pk_st.err, sig_st.err, cls.err, r1_st.err, moff.err, midx.err, mbucket.err,
                       mwin.err, mjac.err})
    if (e != hipSuccess) return (int)e;
  hipError_t e = d_pks.up(pks48, 48 * n);
  if (e == hipSuccess) e = d_sigs.up(sigs96, 96 * n);
  if (e == hipSuccess) e = d_seed.up(seed32, 32);
  if (e != hipSuccess) return (int)e;

  const dim3 blk(KBLOCK), g2(grid_for(2 * n));
  hipLaunchKernelGGL(k_prologue_1<1>, dim3(3 * grid_for(n)), blk, 0, 0, n, (const uint8_t*)d_pks.p,
                     (const uint8_t*)d_sigs.p, (const uint8_t*)d_msgs.p, (uint32_t)32, (const uint8_t*)d_doms.p, 8,
                     (const uint8_t*)d_seed.p, pk_aff.p, pk_st.p, sig_aff.p, sig_st.p, h_aff.p, d_r1.p, r1_st.p,
                     pk_flags, sig_flags);
  hipLaunchKernelGGL(k_rb_g2_test, g2, blk, 0, 0, n, (const uint32_t*)sig_aff.p, sig_st.p, (const uint8_t*)pk_st.p,
                     cls.p, chk);
  hipLaunchKernelGGL(k_rb_msm_sort, dim3((unsigned)nb), blk, 0, 0, n, B, (const uint8_t*)d_seed.p,
                     (const uint8_t*)sig_st.p, (const uint8_t*)pk_st.p, moff.p, midx.p);
  const size_t tasks = nb * RB_MSM_W * (RB_MSM_D - 1);
  hipLaunchKernelGGL(k_rb_msm_bucket, dim3(grid_for(2 * tasks)), blk, 0, 0, n, B, nb, (const uint32_t*)sig_aff.p,
                     (const uint32_t*)moff.p, (const uint16_t*)midx.p, mbucket.p);
  hipLaunchKernelGGL(k_rb_msm_window, dim3(grid_for(2 * nb * RB_MSM_W)), blk, 0, 0, nb, (const uint32_t*)mbucket.p,
                     mwin.p);
  hipLaunchKernelGGL(k_rb_msm_combine, dim3(grid_for(2 * nb)), blk, 0, 0, nb, (const uint32_t*)mwin.p, mjac.p);
  hipLaunchKernelGGL(k_rb_scale_g2, g2, blk, 0, 0, n, (const uint8_t*)d_seed.p, (const uint32_t*)sig_aff.p,
                     (const uint8_t*)sig_st.p, (const uint8_t*)pk_st.p, d_r2.p);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) return (int)e;

  std::vector<uint8_t> h8;
  dev_buf<uint8_t>* sts[4] = {&pk_st, &sig_st, &cls, &r1_st};
  for (int j = 0; j < 4; ++j) {
    if ((e = sts[j]->down(h8)) != hipSuccess) return (int)e;
    std::memcpy(st + j * n, h8.data(), n);
  }
  std::vector<uint32_t> h32;
  if ((e = d_r1.down(h32)) != hipSuccess) return (int)e;
  unsoa_lane(r1, h32, n, 2);
  if ((e = d_r2.down(h32)) != hipSuccess) return (int)e;
  unsoa_pair(r2, h32, n, 3);
  if ((e = moff.down(h32)) != hipSuccess) return (int)e;
  std::memcpy(off, h32.data(), h32.size() * 4);
  std::vector<uint16_t> h16;
  if ((e = midx.down(h16)) != hipSuccess) return (int)e;
  std::memcpy(idx, h16.data(), h16.size() * 2);
  if ((e = mbucket.down(h32)) != hipSuccess) return (int)e;
  unsoa_pair(bucket, h32, nb * RB_MSM_W * RB_MSM_D, 3);
  if ((e = mwin.down(h32)) != hipSuccess) return (int)e;
  unsoa_pair(win, h32, nb * RB_MSM_W, 3);
  if ((e = mjac.down(h32)) != hipSuccess) return (int)e;
  unsoa_pair(sb, h32, nb, 3);
  return 0;
}

}  // extern "C"
