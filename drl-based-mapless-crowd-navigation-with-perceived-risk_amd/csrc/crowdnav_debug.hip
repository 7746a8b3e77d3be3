// crowdnav_debug.hip -- PROFILING BUILD ONLY (build.sh timing -> libcrowdnav_timing.so; the product library has none of this):
// kernels and entry points that put crowdnav_device.h's helpers under test (cn_debug_math, cn_debug_math_n) and known-byte streams
// for counter calibration (cn_calib_launch).  Compiled with the flags of every other unit: -ffp-contract=off is what the
// device-math tests rely on.
#include "crowdnav_device.h"

// ---- device arithmetic under test (PROFILING BUILD ONLY; tests/test_gpu_parity.py::test_device_math_*): the hand-written
// replacements for libm / compiler expansions, one element per thread.  op: 0 cn_sqrt(x)  1 cn_div(x, y)  2 cn_hypot(x, y)
// 3 cn_atan2_t(x, y) = atan2 with x the ordinate (first argument) and y the abscissa  4, 5 sin, cos of cn_det_sincos_t(x)
__global__ void cn_math_kernel(int op, const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ out, int n,
                               const double* __restrict__ trig)
{
    cn_ktab tab = (cn_ktab)trig;           // the env kernels read this table from their kernel-argument block
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r = 0.0, s_, c_;
    switch (op) {
    case 0: r = cn_sqrt(x[i]); break;
    case 1: r = cn_div(x[i], y[i]); break;
    case 2: r = cn_hypot(x[i], y[i]); break;
    case 3: r = cn_atan2_t(tab, x[i], y[i]); break;
    case 4: cn_det_sincos_t(tab, x[i], &s_, &c_); r = s_; break;
    default: cn_det_sincos_t(tab, x[i], &s_, &c_); r = c_; break;
    }
    out[i] = r;
}
extern "C" int cn_debug_math(int op, const double* x, const double* y, double* out, int n, void* stream)
{
    static const double trig[CN_TRIG_COUNT] = CN_TRIG_TABLE;
    double* d = nullptr;
    if (hipMalloc(&d, sizeof(trig)) != hipSuccess) return -1;
    if (hipMemcpy(d, trig, sizeof(trig), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return -1; }
    hipLaunchKernelGGL(cn_math_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, op, x, y, out, n, (const double*)d);
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(d);
    return e == hipSuccess ? 0 : -1;
}

// ---- the roundings, the IoU, the bare-instruction and the wave helpers under test (PROFILING BUILD ONLY;
// tests/test_gpu_device_math.py holds each to Python / numpy, tests/device_math_ref.py).  One element per thread, inputs a..e
// (an op reads only the ones it names), one float64 per element out; `py2` reaches the device functions as they get it in the
// env kernels, a 32-bit flag behind a constant-address-space pointer; `s` is the wave-uniform operand, a kernel scalar.
//    0, 1  cn_round_scaled(a, 1000 | 100)       2, 3  cn_py_round3, cn_py_round2         4, 5  cn_py_round3_t<true>, cn_py_round2_t<true>
//    6, 7  cn_np_around3, cn_np_around2         8, 9  cn_np_around3_t<true>, cn_np_around2_t<true>
//   10, 11 cn_round_np64_2_t<true>, <false>    12, 13 cn_div1000, cn_div100             14 cn_div_z(a, b)
//   15 cn_iou3(a, b, c, d, half = e)           16 cn_iou3_positive (1.0 / 0.0)
//   17, 18 cn_vmin, cn_vmax (a, b)             19 cn_vmax_s(a, s)     20 cn_vclamp(a, b, c)     21 cn_xorsign(a, b)     22 cn_fma_s(a, b, s)
// Wave helpers: n is a multiple of 64 (the host refuses anything else), so every wavefront runs them with all 64 lanes active,
// which is how the env kernels call them.  Integers travel as float64 values, 64-bit words as float64 bit patterns.
//   30, 31 cn_wave_min_d, cn_wave_max_d        32, 33, 34 cn_wave_min_i, cn_wave_max_i, cn_wave_sum_i      35 cn_shfl_xor_d(a, (int)s)
//   40..44 cn_row_shr_i<1, 2, 4, 8, 15>(ident = (int)s, a)         45..49 cn_row_shl_i<1, 2, 4, 8, 15>
//   50 cn_writelane_u64(a, x = b of the wave's lane 0, l)          51 cn_readlane_u64(a, l)       l = the wave's index in the launch mod 64
__global__ void cn_math_n_kernel(int op, const int32_t* __restrict__ flag, double s, const double* __restrict__ a, const double* __restrict__ b,
                                 const double* __restrict__ c, const double* __restrict__ d, const double* __restrict__ e,
                                 double* __restrict__ out, int n)
{
    cn_kflag py2 = (cn_kflag)flag;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int wl = __builtin_amdgcn_readfirstlane(i >> 6) & 63;
    double r = 0.0;
    switch (op) {
    case 0: r = cn_round_scaled(a[i], 1000.0, py2); break;
    case 1: r = cn_round_scaled(a[i], 100.0, py2); break;
    case 2: r = cn_py_round3(a[i], py2); break;
    case 3: r = cn_py_round2(a[i], py2); break;
    case 4: r = cn_py_round3_t<true>(a[i], py2); break;
    case 5: r = cn_py_round2_t<true>(a[i], py2); break;
    case 6: r = cn_np_around3(a[i]); break;
    case 7: r = cn_np_around2(a[i]); break;
    case 8: r = cn_np_around3_t<true>(a[i]); break;
    case 9: r = cn_np_around2_t<true>(a[i]); break;
    case 10: r = cn_round_np64_2_t<true>(a[i], py2); break;
    case 11: r = cn_round_np64_2_t<false>(a[i], py2); break;
    case 12: r = cn_div1000(a[i]); break;
    case 13: r = cn_div100(a[i]); break;
    case 14: r = cn_div_z(a[i], b[i]); break;
    case 15: r = cn_iou3(a[i], b[i], c[i], d[i], e[i], py2); break;
    case 16: r = cn_iou3_positive(a[i], b[i], c[i], d[i], e[i], py2) ? 1.0 : 0.0; break;
    case 17: r = cn_vmin(a[i], b[i]); break;
    case 18: r = cn_vmax(a[i], b[i]); break;
    case 19: r = cn_vmax_s(a[i], s); break;
    case 20: r = cn_vclamp(a[i], b[i], c[i]); break;
    case 21: r = cn_xorsign(a[i], b[i]); break;
    case 22: r = cn_fma_s(a[i], b[i], s); break;
    case 30: r = cn_wave_min_d(a[i]); break;
    case 31: r = cn_wave_max_d(a[i]); break;
    case 32: r = (double)cn_wave_min_i((int)a[i]); break;
    case 33: r = (double)cn_wave_max_i((int)a[i]); break;
    case 34: r = (double)cn_wave_sum_i((int)a[i]); break;
    case 35: r = cn_shfl_xor_d(a[i], (int)s); break;
    case 40: r = (double)cn_row_shr_i<1>((int)s, (int)a[i]); break;
    case 41: r = (double)cn_row_shr_i<2>((int)s, (int)a[i]); break;
    case 42: r = (double)cn_row_shr_i<4>((int)s, (int)a[i]); break;
    case 43: r = (double)cn_row_shr_i<8>((int)s, (int)a[i]); break;
    case 44: r = (double)cn_row_shr_i<15>((int)s, (int)a[i]); break;
    case 45: r = (double)cn_row_shl_i<1>((int)s, (int)a[i]); break;
    case 46: r = (double)cn_row_shl_i<2>((int)s, (int)a[i]); break;
    case 47: r = (double)cn_row_shl_i<4>((int)s, (int)a[i]); break;
    case 48: r = (double)cn_row_shl_i<8>((int)s, (int)a[i]); break;
    case 49: r = (double)cn_row_shl_i<15>((int)s, (int)a[i]); break;
    case 50: r = __longlong_as_double((long long)cn_writelane_u64((unsigned long long)__double_as_longlong(a[i]),
                                                                  (unsigned long long)__double_as_longlong(b[i & ~63]), wl)); break;
    case 51: r = __longlong_as_double((long long)cn_readlane_u64((unsigned long long)__double_as_longlong(a[i]), wl)); break;
    default: break;
    }
    out[i] = r;
}
// a..e: n float64 each on the device (an op's unused inputs may alias a); returns -2 for an op / n it refuses, -1 for a HIP error
extern "C" int cn_debug_math_n(int op, int py2, double s, const double* a, const double* b, const double* c, const double* d, const double* e,
                               double* out, int n, void* stream)
{
    const bool known = (op >= 0 && op <= 22) || (op >= 30 && op <= 35) || (op >= 40 && op <= 51);
    if (!known || n <= 0 || !a || !b || !c || !d || !e || !out) return -2;
    if (op >= 30 && (n & 63) != 0) return -2;          // the wave helpers run under a full exec mask only
    const int32_t flag = py2 ? 1 : 0;
    int32_t* f = nullptr;
    if (hipMalloc(&f, sizeof(flag)) != hipSuccess) return -1;
    if (hipMemcpy(f, &flag, sizeof(flag), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(f); return -1; }
    hipLaunchKernelGGL(cn_math_n_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, op, (const int32_t*)f, s, a, b, c, d, e, out, n);
    const hipError_t err = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(f);
    return err == hipSuccess ? 0 : -1;
}

// ---- PMC calibration (PROFILING BUILD ONLY, libcrowdnav_timing.so; tools/calib_pmc.py): known-byte streaming reads / writes at the access widths the
// env kernel uses, so FETCH_SIZE / WRITE_SIZE can be turned into bytes (MI355X_MICROARCH.md, HBM section).
template <typename T>
__global__ void cn_calib_read_kernel(const T* __restrict__ src, size_t n, T* __restrict__ out)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    T acc = T(0);
    for (; i < n; i += stride) acc += src[i];
    if (acc == T(123456789)) out[0] = acc;  // never true for the zero-filled buffer; keeps the loads alive
}
template <typename T>
__global__ void cn_calib_write_kernel(T* __restrict__ dst, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = T(1);
}
extern "C" void cn_calib_launch(void* buf, size_t bytes, int width, int write, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    dim3 g(256 * 16), b(256);
    if (!write) {
        if (width == 4) hipLaunchKernelGGL(cn_calib_read_kernel<float>, g, b, 0, st, (const float*)buf, bytes / 4, (float*)buf);
        else hipLaunchKernelGGL(cn_calib_read_kernel<double>, g, b, 0, st, (const double*)buf, bytes / 8, (double*)buf);
    } else {
        if (width == 4) hipLaunchKernelGGL(cn_calib_write_kernel<float>, g, b, 0, st, (float*)buf, bytes / 4);
        else hipLaunchKernelGGL(cn_calib_write_kernel<double>, g, b, 0, st, (double*)buf, bytes / 8);
    }
}
