// Device probe of hash_to_G2's try-and-increment searches -- TEST INFRASTRUCTURE.
//
// The search exists in four device forms (pair-sequential, 16-lane wide, known offset, wave-pooled),
// and a search that took a later square or another lane's offset shows only as a False verdict.  This
// translation unit includes bls381_kernels.hpp and launches the product's own kernels, unchanged and
// with the product's workgroup and grid shapes (bls381_capi.hip: launch_hash_g2, launch_hash_koff,
// run_verify's and run_verify_randomized's prologues), and hands what each route wrote back to
// tests/test_hash_search_gpu.py, which compares it with Python integers and
// tests/golden/hash_search.json.  hipcc builds it into lib/libbls381_hashcheck.so.  The library is
// loaded only by tests; the product library (libbls381.so) never links it and it exports no
// bls381_* symbol.
//
// Boundary, as rb_check.hip: host pointers in and out, null stream, nothing left allocated,
// n <= 4096; every Fp crosses raw, as 14 little-endian u32 limb words (28-bit limbs) in the
// Montgomery domain (R = 2^392), nothing converted.  A G2 affine point is (x.c0, x.c1, y.c0, y.c1).
// One entry:
//   hsc_run(n, msgs, mlen, doms, dom_stride, pk48, sig96, cand, koff, bp, st, touched)
//     msgs   n messages of mlen bytes; doms: 8 bytes per item (dom_stride 8) or shared (0)
//     pk48, sig96   one valid key and signature: the decode roles of k_prologue_1 get n copies
//                   (their output is not read)
//     cand   [3][n][4][14]   the candidate (x, y) after root selection, from the h_aff rows of
//                            0: k_hash_cand_1, 1: role 0 of k_prologue_1<0>, 2: of k_prologue_1<1>
//     koff   [n]             k_hash_search<16>
//     bp     [7][n][4][14]   the verification hash BP(H0): 0..2 k_hash_bp over cand 0..2,
//                            3: k_hash_g2_lg<on_octet>, 4: k_hash_g2_lg<on_quad>, 5: k_hash_g2, each
//                            given koff, 6: k_hash_g2 with koff == nullptr (the sequential search)
//     st     [7][n]          the status each of the seven wrote (ST_OK / ST_INF)
//     touched[1]             words written past the n items of any output buffer (each device
//                            buffer carries a guard of GUARD words behind it; all are pre-filled
//                            with 0xFFFFFFFF, which no limb, offset or status equals)
//   Returns 0 or the HIP error code; 0x7fff0000 + i when k_hash_search left item i's offset
//   unwritten or gave one of 64 or more (its consumers step that many times: they are not launched).
#include <cstring>
#include <vector>

#include "bls381.h"   // declarations only (the status codes bls381_kernels.hpp names): nothing here defines them
#include "bls381_kernels.hpp"

using namespace bls381;

namespace {

constexpr size_t MAX_N = 4096;
constexpr size_t GUARD = 1024;

unsigned grid_for(size_t n) { return (unsigned)((n + KBLOCK - 1) / KBLOCK); }

// a device buffer of `count` elements plus the guard, every byte 0xFF, freed on scope exit
template <class T>
struct dev_buf {
  T* p = nullptr;
  size_t count;
  hipError_t err;
  explicit dev_buf(size_t c) : count(c) {
    err = hipMalloc((void**)&p, (count + GUARD) * sizeof(T));
    if (err == hipSuccess) err = hipMemset(p, 0xFF, (count + GUARD) * sizeof(T));
  }
  ~dev_buf() { if (p) (void)hipFree(p); }
  dev_buf(const dev_buf&) = delete;
  dev_buf& operator=(const dev_buf&) = delete;
  hipError_t up(const void* src, size_t bytes) { return hipMemcpy(p, src, bytes, hipMemcpyHostToDevice); }
  // the elements into h, the guard's touched elements added to *touched
  hipError_t down(std::vector<T>& h, uint32_t* touched) {
    h.resize(count + GUARD);
    const hipError_t e = hipMemcpy(h.data(), p, (count + GUARD) * sizeof(T), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (size_t k = count; k < count + GUARD; ++k)
      if (h[k] != (T)~(T)0) ++*touched;
    h.resize(count);
    return e;
  }
};

// lane-pair SoA -> item-major: limb k of Fp2 component c, coefficient p, at src[(c 14 + k) 2 n + 2 i + p]
void unsoa_pair(uint32_t* dst, const std::vector<uint32_t>& src, size_t n) {
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 2; ++c)
      for (int p = 0; p < 2; ++p)
        for (int k = 0; k < FP_LIMBS; ++k)
          dst[((i * 2 + c) * 2 + p) * FP_LIMBS + k] = src[(size_t)(c * FP_LIMBS + k) * 2 * n + 2 * i + p];
}

hipError_t settle() {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}

}  // namespace

extern "C" {

int hsc_run(size_t n, const uint8_t* msgs, uint32_t mlen, const uint8_t* doms, int dom_stride, const uint8_t* pk48,
            const uint8_t* sig96, uint32_t* cand, uint32_t* koff, uint32_t* bp, uint8_t* st, uint32_t* touched) {
  if (n == 0 || n > MAX_N || mlen == 0 || mlen > 1024 || (dom_stride != 0 && dom_stride != 8))
    return (int)hipErrorInvalidValue;
  if (!msgs || !doms || !pk48 || !sig96 || !cand || !koff || !bp || !st || !touched) return (int)hipErrorInvalidValue;
  *touched = 0;
  const size_t pt = 4 * FP_LIMBS * n;   // words of n G2 affine points
  const size_t ndom = dom_stride ? n : 1;

  dev_buf<uint8_t> d_msgs((size_t)mlen * n), d_doms(8 * ndom), d_pks(48 * n), d_sigs(96 * n), d_seed(32);
  dev_buf<uint32_t> h0(pt), h1(pt), h2(pt), h3(pt), h4(pt), h5(pt), h6(pt), d_koff(n);
  dev_buf<uint8_t> s0(n), s1(n), s2(n), s3(n), s4(n), s5(n), s6(n);
  // the decode roles' outputs (not read)
  dev_buf<uint32_t> pk_aff(2 * FP_LIMBS * n), sig_aff(pt), r1(2 * FP_LIMBS * n);
  dev_buf<uint8_t> pk_st(n), sig_st(n), r1_st(n);
  dev_buf<uint32_t>* hs[7] = {&h0, &h1, &h2, &h3, &h4, &h5, &h6};
  dev_buf<uint8_t>* ss[7] = {&s0, &s1, &s2, &s3, &s4, &s5, &s6};
  for (hipError_t e : {d_msgs.err, d_doms.err, d_pks.err, d_sigs.err, d_seed.err, h0.err, h1.err, h2.err, h3.err,
                       h4.err, h5.err, h6.err, d_koff.err, s0.err, s1.err, s2.err, s3.err, s4.err, s5.err, s6.err,
                       pk_aff.err, sig_aff.err, r1.err, pk_st.err, sig_st.err, r1_st.err})
    if (e != hipSuccess) return (int)e;
  std::vector<uint8_t> rep(96 * n);
  hipError_t e = d_msgs.up(msgs, (size_t)mlen * n);
  if (e == hipSuccess) e = d_doms.up(doms, 8 * ndom);
  for (size_t i = 0; i < n; ++i) std::memcpy(&rep[48 * i], pk48, 48);
  if (e == hipSuccess) e = d_pks.up(rep.data(), 48 * n);
  for (size_t i = 0; i < n; ++i) std::memcpy(&rep[96 * i], sig96, 96);
  if (e == hipSuccess) e = d_sigs.up(rep.data(), 96 * n);
  if (e == hipSuccess) e = hipMemset(d_seed.p, 0x5A, 32);
  if (e != hipSuccess) return (int)e;

  const dim3 blk(KBLOCK), g1(grid_for(n)), g2(grid_for(2 * n)), g3(3 * grid_for(n));
  const uint8_t* m = d_msgs.p;
  const uint8_t* d = d_doms.p;
  std::vector<uint32_t> h32;
  std::vector<uint8_t> h8;

  // ---- the pooled search: three launches, each followed by the cofactor map in place
  for (int j = 0; j < 3; ++j) {
    uint32_t* h = hs[j]->p;
    if (j == 0)
      hipLaunchKernelGGL(k_hash_cand_1, g1, blk, 0, 0, n, m, mlen, d, dom_stride, h);
    else if (j == 1)
      hipLaunchKernelGGL(k_prologue_1<0>, g3, blk, 0, 0, n, (const uint8_t*)d_pks.p, (const uint8_t*)d_sigs.p, m, mlen,
                         d, dom_stride, (const uint8_t*)nullptr, pk_aff.p, pk_st.p, sig_aff.p, sig_st.p, h,
                         (uint32_t*)nullptr, (uint8_t*)nullptr, (int)CHK_LAX, (int)CHK_LAX);
    else
      hipLaunchKernelGGL(k_prologue_1<1>, g3, blk, 0, 0, n, (const uint8_t*)d_pks.p, (const uint8_t*)d_sigs.p, m, mlen,
                         d, dom_stride, (const uint8_t*)d_seed.p, pk_aff.p, pk_st.p, sig_aff.p, sig_st.p, h, r1.p,
                         r1_st.p, 1, 0);
    if ((e = settle()) != hipSuccess) return (int)e;
    if ((e = hs[j]->down(h32, touched)) != hipSuccess) return (int)e;
    unsoa_pair(cand + (size_t)j * pt, h32, n);
    hipLaunchKernelGGL(k_hash_bp, g2, blk, 0, 0, n, h, ss[j]->p);
    if ((e = settle()) != hipSuccess) return (int)e;
  }

  // ---- the wide search, its three consumers, and the sequential search
  hipLaunchKernelGGL(k_hash_search<16>, dim3(grid_for(16 * n)), blk, 0, 0, n, m, mlen, d, dom_stride, d_koff.p);
  if ((e = settle()) != hipSuccess) return (int)e;
  if ((e = d_koff.down(h32, touched)) != hipSuccess) return (int)e;
  std::memcpy(koff, h32.data(), 4 * n);
  // an offset the search did not write stays out of the consumers (they would loop over it)
  for (size_t i = 0; i < n; ++i)
    if (koff[i] >= 64) return 0x7fff0000 + (int)i;
  const uint32_t* ko = d_koff.p;
  hipLaunchKernelGGL(k_hash_g2_lg<on_octet>, dim3(grid_for(8 * n)), blk, 0, 0, n, m, mlen, d, dom_stride, h3.p, s3.p, ko, 0);
  if ((e = settle()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_hash_g2_lg<on_quad>, dim3(grid_for(4 * n)), blk, 0, 0, n, m, mlen, d, dom_stride, h4.p, s4.p, ko, 0);
  if ((e = settle()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_hash_g2, g2, blk, 0, 0, n, m, mlen, d, dom_stride, h5.p, s5.p, ko, 0);
  if ((e = settle()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_hash_g2, g2, blk, 0, 0, n, m, mlen, d, dom_stride, h6.p, s6.p, (const uint32_t*)nullptr, 0);
  if ((e = settle()) != hipSuccess) return (int)e;

  for (int j = 0; j < 7; ++j) {
    if ((e = hs[j]->down(h32, touched)) != hipSuccess) return (int)e;
    unsoa_pair(bp + (size_t)j * pt, h32, n);
    if ((e = ss[j]->down(h8, touched)) != hipSuccess) return (int)e;
    std::memcpy(st + (size_t)j * n, h8.data(), n);
  }
  return 0;
}

}  // extern "C"
