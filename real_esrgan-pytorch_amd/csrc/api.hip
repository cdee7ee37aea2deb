// api.hip -- the extern "C" boundary of libresr_hip.so (declared in include/resr.h).
// Plain pointers and sizes only; no torch / ATen types; errors become negative status codes plus a
// thread-local message.  Every entry point enqueues on the caller's stream and returns.
#include <stdarg.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "host_api.h"
#include "packed_layout.h"

namespace resr {

char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

// ---- in-situ profiling -------------------------------------------------------------------------------------
// Launches come from the Python main thread (forward) and from autograd worker threads (backward): the record list is
// guarded by a mutex, the switch is atomic, and the "before" event of a launch lives in the launching thread.
namespace {
struct ProfRec { hipEvent_t e0, e1; int id; double flop, bytes; };
std::vector<ProfRec> g_prof;
std::mutex g_prof_mu;
std::atomic<bool> g_prof_on{false};
thread_local hipEvent_t t_prof_e0 = nullptr;
}  // namespace
bool prof_on() { return g_prof_on.load(std::memory_order_relaxed); }
void prof_before(hipStream_t st) {
    if (!prof_on()) return;
    (void)hipEventCreate(&t_prof_e0);
    (void)hipEventRecord(t_prof_e0, st);
}
void prof_after(hipStream_t st, int kernel_id, double flop, double bytes) {
    if (!prof_on() || !t_prof_e0) return;
    ProfRec r;
    r.e0 = t_prof_e0; r.id = kernel_id; r.flop = flop; r.bytes = bytes;
    (void)hipEventCreate(&r.e1);
    (void)hipEventRecord(r.e1, st);
    t_prof_e0 = nullptr;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof.push_back(r);
}

// Every entry point runs on the device that owns the caller's stream, whatever the calling thread's current device is
// (the boundary is used from the Python main thread and from autograd worker threads, one process per GPU or not):
// hipStreamGetDevice names it, the scope switches to it and back.  The null stream means "the current device".
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(void* stream) {
        if (!stream) return;
        hipDevice_t dev = 0;
        int cur = 0;
        if (hipStreamGetDevice((hipStream_t)stream, &dev) != hipSuccess || hipGetDevice(&cur) != hipSuccess) return;
        if ((int)dev != cur && hipSetDevice((int)dev) == hipSuccess) prev = cur;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
#define RESR_DEVICE_SCOPE(stream) DeviceScope resr_device_scope_(stream)

// probe used by tests: what does ds_read_b64_tr_b16 hand to (lane, element)?  LDS holds the element
// index at every position; lane l supplies byte address l*8.
typedef __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16 fp16x4_t;
__global__ void tr_probe_kernel(float* out) {
    __shared__ __attribute__((aligned(16))) _Float16 lds[256];
    const int l = threadIdx.x;
    for (int i = l; i < 256; i += 64) lds[i] = (_Float16)i;
    __syncthreads();
    auto p = reinterpret_cast<__attribute__((address_space(3))) fp16x4_t*>(
        (__attribute__((address_space(3))) _Float16*)(lds + l * 4));
    const fp16x4_t r = __builtin_amdgcn_ds_read_tr16_b64_v4f16(p);
    for (int j = 0; j < 4; ++j) out[l * 4 + j] = (float)r[j];
}

// test aid: `workgroups` workgroups that each hold `lds_bytes` of LDS and spin for `micros` microseconds -- what a collective
// kernel of another stream looks like to a chained launch that needs every CU (tests/test_gpu_chain.py)
__global__ void occupy_kernel(unsigned long long ticks, unsigned* sink) {
    extern __shared__ unsigned occ_lds[];
    occ_lds[threadIdx.x] = threadIdx.x;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
    if (sink && occ_lds[threadIdx.x] == 0xffffffffu) *sink = 1;
}

}  // namespace resr

using namespace resr;

extern "C" {

int resr_version(void) { return RESR_VERSION; }
const char* resr_last_error(void) { return err_buf(); }

int resr_conv3x3(const ResrConvDesc* d, const void* in0, const void* in1, const void* w_packed, const float* bias,
                 const void* res0, const void* res1, const void* mask, void* out, void* aux_out, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return conv3x3_dispatch(d, in0, in1, w_packed, bias, res0, res1, mask, out, aux_out, (hipStream_t)stream);
}

int resr_conv3x3_chain(int32_t njobs, const ResrConvDesc* descs, const void* in0, const void* in1,
                       const void* const* packed_w, const float* const* bias, const void* const* mask,
                       void* const* out, void* const* aux_out, void* chain_state, size_t chain_state_bytes, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    if (!descs || !in0 || !packed_w || !out) return fail(RESR_ERR_ARG, "conv3x3_chain: null argument");
    return conv3x3_chain_dispatch(njobs, descs, in0, in1, packed_w, bias, mask, out, aux_out, chain_state, chain_state_bytes, (hipStream_t)stream);
}

size_t resr_conv3x3_chain_state_bytes(int32_t n, int32_t h, int32_t w) { return conv3x3_chain_state_bytes(n, h, w); }

size_t resr_wgrad_partial_bytes(const ResrWgradDesc* d) { return d ? wgrad_partial_bytes(d) : 0; }

int resr_conv3x3_wgrad(const ResrWgradDesc* d, const void* x0, const void* x1, const void* g, float* partial,
                       float* dw, float* db, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return wgrad_dispatch(d, x0, x1, g, partial, dw, db, (hipStream_t)stream);
}

// test entry of the sparse-tap weight gradient (tests/test_gpu_sparse_taps.py): resr_conv3x3_wgrad on a space-to-depth X
int resr_debug_conv3x3_wgrad_s2d(const ResrWgradDesc* d, const void* x0, const void* x1, const void* g, float* partial,
                                 float* dw, float* db, int32_t x_s2d_c, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return wgrad_debug_s2d(d, x0, x1, g, partial, dw, db, x_s2d_c, (hipStream_t)stream);
}

int resr_pack_weights(const ResrPackChunk* chunks_dev, int32_t n_chunks, const float* arena, void* packed,
                      int32_t dtype, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return pack_dispatch(chunks_dev, n_chunks, arena, packed, dtype, (hipStream_t)stream);
}

int resr_pack_weights_mx(const ResrPackChunk* chunks_dev, int32_t n_chunks, const float* arena, void* packed_mx, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return pack_mx_dispatch(chunks_dev, n_chunks, arena, packed_mx, (hipStream_t)stream);
}

int64_t resr_conv_pack_table(int32_t cout, int32_t cin, int32_t transposed, int64_t src_off, int64_t dst_off, float scale, ResrPackChunk* chunks,
                             int64_t capacity) {
    if (cout <= 0 || cin <= 0 || (transposed != 0 && transposed != 1)) return fail(RESR_ERR_ARG, "conv_pack_table: cout=%d cin=%d transposed=%d", cout, cin, transposed);
    std::vector<ResrPackChunk> t;
    emit_conv_chunks(t, src_off, cout, cin, transposed, dst_off, scale);
    return copy_pack_table(t, chunks, capacity, "conv_pack_table");
}
int64_t resr_conv_packed_elems(int32_t cout, int32_t cin) { return cout > 0 && cin > 0 ? (int64_t)packed_conv_elems(round32(cout), round32(cin)) : 0; }
size_t resr_packed_bytes(int64_t elems, int32_t dtype) { return packed_buffer_bytes((size_t)elems, dtype); }
size_t resr_packed_mx_offset(int64_t elems) { return packed_mx_offset((size_t)elems); }

int resr_nchw_to_nhwc(const float* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t unshuffle,
                      int32_t c_pad, int32_t dtype, const uint8_t* mask, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return nchw_to_nhwc_dispatch(src, dst, n, c, h, w, unshuffle, c_pad, dtype, mask, (hipStream_t)stream, -1L);
}

int resr_nhwc_to_nchw(const void* src, float* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t shuffle,
                      int32_t src_stride, int32_t dtype, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return nhwc_to_nchw_dispatch(src, dst, n, c, h, w, shuffle, src_stride, dtype, (hipStream_t)stream, -1L);
}

int resr_sumpool2x2(const void* src, void* dst, const void* mask, int32_t n, int32_t h_out, int32_t w_out, int32_t c,
                    int32_t dtype, float slope, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return sumpool2x2_dispatch(src, dst, mask, n, h_out, w_out, c, dtype, slope, (hipStream_t)stream, -1L, -1L);
}

size_t resr_generator_param_count(const ResrGeneratorDesc* d) { return generator_param_count(d); }
size_t resr_generator_packed_bytes(const ResrGeneratorDesc* d, int32_t backward) { return generator_packed_bytes(d, backward); }
size_t resr_generator_mx_offset(const ResrGeneratorDesc* d) { return generator_mx_offset(d); }
size_t resr_generator_workspace_bytes(const ResrGeneratorDesc* d) { return generator_workspace_bytes(d); }
size_t resr_generator_chain_state_bytes(const ResrGeneratorDesc* d) { return generator_chain_state_bytes(d); }
int64_t resr_generator_pack_table(const ResrGeneratorDesc* d, int32_t backward, ResrPackChunk* chunks, int64_t capacity) {
    return generator_pack_table(d, backward, chunks, capacity);
}

int64_t resr_generator_buffer_offsets(const ResrGeneratorDesc* d, int64_t* out, int64_t capacity) {
    return generator_buffer_offsets(d, out, capacity);
}

int resr_generator_forward(const ResrGeneratorDesc* d, const float* x_nchw, const float* params, const void* packed,
                           void* workspace, size_t workspace_bytes, float* y_nchw, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return generator_forward(d, x_nchw, params, packed, workspace, workspace_bytes, y_nchw, (hipStream_t)stream);
}

int resr_generator_backward(const ResrGeneratorDesc* d, const float* gy_nchw, const float* params, const void* packed,
                            void* workspace, size_t workspace_bytes, float* grad_params, float* gx_nchw, void* stream,
                            void* const* grad_ready_events, int32_t n_events) {
    RESR_DEVICE_SCOPE(stream);
    return generator_backward(d, gy_nchw, params, packed, workspace, workspace_bytes, grad_params, gx_nchw,
                              (hipStream_t)stream, grad_ready_events, n_events);
}

size_t resr_compact_param_count(const ResrCompactDesc* d) { return compact_param_count(d); }
size_t resr_compact_packed_bytes(const ResrCompactDesc* d) { return compact_packed_bytes(d); }
size_t resr_compact_workspace_bytes(const ResrCompactDesc* d) { return compact_workspace_bytes(d); }
int64_t resr_compact_pack_table(const ResrCompactDesc* d, ResrPackChunk* chunks, int64_t capacity) {
    return compact_pack_table(d, chunks, capacity);
}

int resr_compact_forward(const ResrCompactDesc* d, const float* x_nchw, const float* params, const void* packed,
                         void* workspace, size_t workspace_bytes, float* y_nchw, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_forward_ends(d, {END_F32, false, x_nchw, y_nchw, {}, nullptr, nullptr, 0}, params, packed, workspace, workspace_bytes, (hipStream_t)stream,
                                "compact_forward");
}

size_t resr_compact_train_packed_bytes(const ResrCompactDesc* d) { return compact_train_packed_bytes(d); }
int64_t resr_compact_train_pack_table(const ResrCompactDesc* d, ResrPackChunk* chunks, int64_t capacity) { return compact_train_pack_table(d, chunks, capacity); }
size_t resr_compact_train_workspace_bytes(const ResrCompactDesc* d) { return compact_train_workspace_bytes(d); }
size_t resr_compact_train_state_bytes(const ResrCompactDesc* d) { return compact_train_state_bytes(d); }

int resr_compact_forward_train(const ResrCompactDesc* d, const float* x_nchw, const float* params, const void* packed,
                               void* workspace, size_t workspace_bytes, float* y_nchw, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_forward_train(d, x_nchw, params, packed, workspace, workspace_bytes, y_nchw, (hipStream_t)stream);
}

int resr_compact_backward(const ResrCompactDesc* d, const float* gy_nchw, const float* params, const void* packed,
                          void* workspace, size_t workspace_bytes, float* grad_params, float* gx_nchw, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_backward(d, gy_nchw, params, packed, workspace, workspace_bytes, grad_params, gx_nchw, (hipStream_t)stream);
}

int resr_compact_forward_u8(const ResrCompactDesc* d, const uint8_t* x_u8, const float* params, const void* packed,
                            void* workspace, size_t workspace_bytes, uint8_t* y_u8, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_forward_ends(d, {END_IMAGE, false, x_u8, y_u8, {}, nullptr, nullptr, 0, &kRgb8}, params, packed, workspace, workspace_bytes, (hipStream_t)stream,
                                "compact_forward_u8");
}

int resr_compact_forward_u8_scaled(const ResrCompactDesc* d, const uint8_t* x_u8, const float* params, const void* packed,
                                   void* workspace, size_t workspace_bytes, uint8_t* y_u8, int32_t oh, int32_t ow,
                                   const int32_t* idx_y, const float* w_y, int32_t taps_y, const int32_t* idx_x, const float* w_x,
                                   int32_t taps_x, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_forward_ends(d, {END_IMAGE, true, x_u8, y_u8, {oh, ow, taps_y, taps_x, idx_y, idx_x, w_y, w_x}, nullptr, nullptr, 0, &kRgb8}, params, packed,
                                workspace, workspace_bytes, (hipStream_t)stream, "compact_forward_u8_scaled");
}

int resr_image_resize(const float* src_f32, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow,
                      const int32_t* idx_y, const float* w_y, int32_t taps_y, const int32_t* idx_x, const float* w_x, int32_t taps_x,
                      int32_t out_u8, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return image_resize_dispatch(src_f32, dst, n, c, h, w, oh, ow, idx_y, w_y, taps_y, idx_x, w_x, taps_x, out_u8, (hipStream_t)stream);
}

int resr_u8_to_nchw(const uint8_t* src_u8, float* dst_f32, int32_t n, int32_t h, int32_t w, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return u8_to_nchw_dispatch(src_u8, dst_f32, n, h, w, (hipStream_t)stream);
}

int resr_nchw_to_u8(const float* src_f32, uint8_t* dst_u8, int32_t n, int32_t h, int32_t w, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return nchw_to_u8_dispatch(src_f32, dst_u8, n, h, w, (hipStream_t)stream);
}

int resr_compact_forward_image(const ResrCompactDesc* d, const void* x, const float* params, const void* packed, void* workspace,
                               size_t workspace_bytes, void* y, const ResrImageDesc* img, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_forward_ends(d, {END_IMAGE, false, x, y, {}, nullptr, nullptr, 0, img}, params, packed, workspace, workspace_bytes, (hipStream_t)stream,
                                "compact_forward_image");
}

int resr_compact_forward_image_scaled(const ResrCompactDesc* d, const void* x, const float* params, const void* packed, void* workspace,
                                      size_t workspace_bytes, void* y, int32_t oh, int32_t ow, const int32_t* idx_y, const float* w_y,
                                      int32_t taps_y, const int32_t* idx_x, const float* w_x, int32_t taps_x, const ResrImageDesc* img,
                                      void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_forward_ends(d, {END_IMAGE, true, x, y, {oh, ow, taps_y, taps_x, idx_y, idx_x, w_y, w_x}, nullptr, nullptr, 0, img}, params, packed,
                                workspace, workspace_bytes, (hipStream_t)stream, "compact_forward_image_scaled");
}

int resr_compact_image_scaled_fits(int32_t h, int32_t w, int32_t s, int32_t oh, int32_t ow, int32_t taps_y, int32_t taps_x, int32_t channels,
                                   int32_t bits) {
    ResizeGeom g;
    int kind;
    return image_scaled_plan(h, w, s, oh, ow, taps_y, taps_x, channels, bits, &g, &kind) ? 1 : 0;
}

int resr_image_to_nchw(const void* src, float* dst_f32, int32_t n_images, int32_t h, int32_t w, const ResrImageDesc* img, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return image_to_nchw_dispatch(src, dst_f32, n_images, h, w, img, (hipStream_t)stream);
}

int resr_nchw_to_image(const float* src_f32, void* dst, int32_t n_images, int32_t h, int32_t w, const ResrImageDesc* img, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return nchw_to_image_dispatch(src_f32, dst, n_images, h, w, img, (hipStream_t)stream);
}

int resr_compact_forward_yuv420(const ResrCompactDesc* d, const uint8_t* x_yuv, const float* params, const void* packed,
                                void* workspace, size_t workspace_bytes, uint8_t* y_yuv, const ResrYuvDesc* yuv, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_forward_ends(d, {END_YUV, false, x_yuv, y_yuv, {}, yuv, yuv, 8}, params, packed, workspace, workspace_bytes, (hipStream_t)stream,
                                "compact_forward_yuv420");
}

int resr_yuv420_to_rgb(const uint8_t* src, uint8_t* dst_hwc, int32_t n, int32_t h, int32_t w, const ResrYuvDesc* yuv, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return yuv420_to_rgb_dispatch(src, dst_hwc, n, h, w, yuv, (hipStream_t)stream);
}

int resr_rgb_to_yuv420(const uint8_t* src_hwc, uint8_t* dst, int32_t n, int32_t h, int32_t w, const ResrYuvDesc* yuv, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return rgb_to_yuv420_dispatch(src_hwc, dst, n, h, w, yuv, (hipStream_t)stream);
}

int resr_compact_forward_yuv420p10(const ResrCompactDesc* d, const uint16_t* x_yuv, const float* params, const void* packed,
                                   void* workspace, size_t workspace_bytes, uint16_t* y_yuv, const ResrYuvDesc* yuv, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_forward_ends(d, {END_YUV, false, x_yuv, y_yuv, {}, yuv, yuv, 10}, params, packed, workspace, workspace_bytes, (hipStream_t)stream,
                                "compact_forward_yuv420p10");
}

int resr_yuv420p10_to_nchw(const uint16_t* src, float* dst_f32, int32_t n, int32_t h, int32_t w, const ResrYuvDesc* yuv, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return yuv420p10_to_nchw_dispatch(src, dst_f32, n, h, w, yuv, (hipStream_t)stream);
}

int resr_nchw_to_yuv420p10(const float* src_f32, uint16_t* dst, int32_t n, int32_t h, int32_t w, const ResrYuvDesc* yuv, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return nchw_to_yuv420p10_dispatch(src_f32, dst, n, h, w, yuv, (hipStream_t)stream);
}

int resr_compact_forward_yuv420_scaled(const ResrCompactDesc* d, const uint8_t* x_yuv, const float* params, const void* packed,
                                       void* workspace, size_t workspace_bytes, uint8_t* y_yuv, int32_t oh, int32_t ow,
                                       const int32_t* idx_y, const float* w_y, int32_t taps_y, const int32_t* idx_x, const float* w_x,
                                       int32_t taps_x, const ResrYuvDesc* yuv, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_forward_ends(d, {END_YUV, true, x_yuv, y_yuv, {oh, ow, taps_y, taps_x, idx_y, idx_x, w_y, w_x}, yuv, yuv, 8}, params, packed,
                                workspace, workspace_bytes, (hipStream_t)stream, "compact_forward_yuv420_scaled");
}

int resr_compact_forward_yuv420p10_scaled(const ResrCompactDesc* d, const uint16_t* x_yuv, const float* params, const void* packed,
                                          void* workspace, size_t workspace_bytes, uint16_t* y_yuv, int32_t oh, int32_t ow,
                                          const int32_t* idx_y, const float* w_y, int32_t taps_y, const int32_t* idx_x, const float* w_x,
                                          int32_t taps_x, const ResrYuvDesc* yuv, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_forward_ends(d, {END_YUV, true, x_yuv, y_yuv, {oh, ow, taps_y, taps_x, idx_y, idx_x, w_y, w_x}, yuv, yuv, 10}, params, packed,
                                workspace, workspace_bytes, (hipStream_t)stream, "compact_forward_yuv420p10_scaled");
}

int resr_compact_forward_yuv420_mixed(const ResrCompactDesc* d, const void* x_yuv, const ResrYuvDesc* src_yuv, const float* params,
                                      const void* packed, void* workspace, size_t workspace_bytes, void* y_yuv,
                                      const ResrYuvDesc* dst_yuv, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_forward_ends(d, {END_YUV, false, x_yuv, y_yuv, {}, src_yuv, dst_yuv, 0}, params, packed, workspace, workspace_bytes,
                                (hipStream_t)stream, "compact_forward_yuv420_mixed");
}

int resr_compact_forward_yuv420_mixed_scaled(const ResrCompactDesc* d, const void* x_yuv, const ResrYuvDesc* src_yuv, const float* params,
                                             const void* packed, void* workspace, size_t workspace_bytes, void* y_yuv, int32_t oh,
                                             int32_t ow, const int32_t* idx_y, const float* w_y, int32_t taps_y, const int32_t* idx_x,
                                             const float* w_x, int32_t taps_x, const ResrYuvDesc* dst_yuv, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_forward_ends(d, {END_YUV, true, x_yuv, y_yuv, {oh, ow, taps_y, taps_x, idx_y, idx_x, w_y, w_x}, src_yuv, dst_yuv, 0}, params,
                                packed, workspace, workspace_bytes, (hipStream_t)stream, "compact_forward_yuv420_mixed_scaled");
}

int resr_compact_yuv420_scaled_fits(int32_t h, int32_t w, int32_t s, int32_t oh, int32_t ow, int32_t taps_y, int32_t taps_x, int32_t bits) {
    return compact_yuv420_scaled_fits(h, w, s, oh, ow, taps_y, taps_x, bits);
}

size_t resr_discriminator_param_count(void) { return discriminator_param_count(); }
size_t resr_discriminator_uv_count(void) { return discriminator_uv_count(); }
size_t resr_discriminator_workspace_bytes(const ResrDiscriminatorDesc* d) { return discriminator_workspace_bytes(d); }
int64_t resr_discriminator_pack_table(const ResrDiscriminatorDesc* d, const void* workspace, ResrPackChunk* chunks, int64_t capacity) {
    return discriminator_pack_table(d, workspace, chunks, capacity);
}

int resr_discriminator_forward(const ResrDiscriminatorDesc* d, const float* x_nchw, const float* params, float* uv,
                               const ResrPackChunk* table_dev, int32_t n_chunks, void* workspace, size_t workspace_bytes,
                               float* y_nchw, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return discriminator_forward(d, x_nchw, params, uv, table_dev, n_chunks, workspace, workspace_bytes, y_nchw, (hipStream_t)stream);
}

int resr_discriminator_backward(const ResrDiscriminatorDesc* d, const float* gy_nchw, const float* params, void* workspace,
                                size_t workspace_bytes, float* grad_params, float* gx_nchw, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return discriminator_backward(d, gy_nchw, params, workspace, workspace_bytes, grad_params, gx_nchw, (hipStream_t)stream);
}

int resr_discriminator_backward_f16(const ResrDiscriminatorDesc* d, const float* gy_nchw, const float* params,
                                    const ResrPackChunk* table_dev, int32_t n_chunks, void* workspace, size_t workspace_bytes,
                                    float* grad_params, float* gx_nchw, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return discriminator_backward_f16(d, gy_nchw, params, table_dev, n_chunks, workspace, workspace_bytes, grad_params, gx_nchw,
                                      (hipStream_t)stream);
}

int resr_ema_update(float* shadow, const float* params, int64_t count, double decay, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return ema_dispatch(shadow, params, (long)count, decay, (hipStream_t)stream);
}

int resr_tile_batch(const uint8_t* tiles, const int32_t* index, const uint8_t* aug, int32_t m, int32_t b, int32_t t, float* dst, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return tile_batch_dispatch(tiles, index, aug, m, b, t, dst, (hipStream_t)stream);
}

int resr_blur_kernels(const double* params, int32_t n, int32_t k, float* dst, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return blur_kernels_dispatch(params, n, k, dst, (hipStream_t)stream);
}

int resr_pair_batch(const uint8_t* hr_arena, const uint8_t* lr_arena, const int64_t* table, const int32_t* records, int32_t m, int32_t b, int32_t patch,
                    int32_t scale, float* lr_dst, float* hr_dst, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return pair_batch_dispatch(hr_arena, lr_arena, table, records, m, b, patch, scale, lr_dst, hr_dst, (hipStream_t)stream);
}

int resr_crop_batch(const uint8_t* arena, const int64_t* table, const int32_t* records, int32_t m, int32_t b, int32_t t, float* dst, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return crop_batch_dispatch(arena, table, records, m, b, t, dst, (hipStream_t)stream);
}

int resr_pool_exchange(float* pool_lr, float* pool_hr, const float* lr_in, const float* hr_in, float* lr_out, float* hr_out, const int32_t* slots, int32_t q,
                       int32_t b, int64_t lr_elems, int64_t hr_elems, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return pool_exchange_dispatch(pool_lr, pool_hr, lr_in, hr_in, lr_out, hr_out, slots, q, b, lr_elems, hr_elems, (hipStream_t)stream);
}

int resr_resample_ksize(int64_t in_size, int64_t out_size) { return resample_ksize(in_size, out_size); }

int resr_resample_tables(int64_t in_size, int64_t out_size, int32_t* bounds, int32_t* coeffs, int32_t ksize_capacity) {
    return resample_tables(in_size, out_size, bounds, coeffs, ksize_capacity);
}

int resr_resample_u8(uint8_t* arena, int64_t arena_bytes, const int64_t* jobs_host, const int64_t* jobs_dev, int32_t j, const int32_t* tables, int64_t table_words,
                     void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return resample_u8_dispatch(arena, arena_bytes, jobs_host, jobs_dev, j, tables, table_words, (hipStream_t)stream);
}

int resr_niqe_luma_f32(const float* src, uint8_t* dst, int32_t n, int32_t h, int32_t w, int32_t crop, int32_t out_h, int32_t out_w, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return niqe_luma_dispatch(src, 0, dst, n, h, w, crop, out_h, out_w, (hipStream_t)stream);
}

int resr_niqe_luma_u8(const uint8_t* src, uint8_t* dst, int32_t n, int32_t h, int32_t w, int32_t crop, int32_t out_h, int32_t out_w, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return niqe_luma_dispatch(src, 1, dst, n, h, w, crop, out_h, out_w, (hipStream_t)stream);
}

size_t resr_niqe_workspace_bytes(const ResrNiqeDesc* d) { return niqe_workspace_bytes(d); }

int resr_niqe_features(const ResrNiqeDesc* d, const uint8_t* luma, double* feats, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return niqe_features_dispatch(d, luma, feats, (hipStream_t)stream);
}

size_t resr_niqe_score_workspace_bytes(const ResrNiqeScoreDesc* d) { return niqe_score_workspace_bytes(d); }

int resr_niqe_score(const ResrNiqeScoreDesc* d, const double* feats, double* scores, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return niqe_score_dispatch(d, feats, scores, (hipStream_t)stream);
}

size_t resr_fullref_workspace_bytes(const ResrFullRefDesc* d) { return fullref_workspace_bytes(d); }

int resr_fullref(const ResrFullRefDesc* d, const void* sr, const void* hr, int64_t* sse, double* psnr, double* ssim, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return fullref_dispatch(d, sr, hr, sse, psnr, ssim, (hipStream_t)stream);
}

size_t resr_jpeg_encode_max_bytes(const ResrJpegEncDesc* d) { return jpeg_encode_max_bytes(d); }

size_t resr_jpeg_encode_workspace_bytes(const ResrJpegEncDesc* d) { return jpeg_encode_workspace_bytes(d); }

int resr_jpeg_encode_header(const ResrJpegEncDesc* d, uint8_t* host_buf, size_t cap) { return jpeg_encode_header(d, host_buf, cap); }

int resr_jpeg_encode(const ResrJpegEncDesc* d, const uint8_t* rgb_hwc, uint8_t* out, int64_t out_stride, int64_t* lengths, const uint8_t* header_dev, int32_t header_len,
                     void* workspace, size_t workspace_bytes, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return jpeg_encode_dispatch(d, rgb_hwc, out, out_stride, lengths, header_dev, header_len, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t resr_png_encode_max_bytes(const ResrPngEncDesc* d) { return png_encode_max_bytes(d); }

size_t resr_png_encode_workspace_bytes(const ResrPngEncDesc* d) { return png_encode_workspace_bytes(d); }

int resr_png_encode_header(const ResrPngEncDesc* d, uint8_t* host_buf, size_t cap) { return png_encode_header(d, host_buf, cap); }

int resr_png_encode(const ResrPngEncDesc* d, const void* src, uint8_t* out, int64_t out_stride, int64_t* lengths, const uint8_t* header_dev, int32_t header_bytes, void* workspace,
                    size_t workspace_bytes, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return png_encode_dispatch(d, src, out, out_stride, lengths, header_dev, header_bytes, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t resr_png_debug_deflate_workspace_bytes(int64_t stream_bytes, int32_t segment_bytes) { return png_debug_deflate_workspace_bytes(stream_bytes, segment_bytes); }

int resr_png_debug_deflate(const uint8_t* stream_dev, int64_t stream_bytes, int32_t segment_bytes, uint8_t* out, int64_t out_capacity, int64_t* length, void* workspace,
                           size_t workspace_bytes, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return png_debug_deflate(stream_dev, stream_bytes, segment_bytes, out, out_capacity, length, workspace, workspace_bytes, (hipStream_t)stream);
}

int resr_png_debug_build_code(const uint32_t* counts_dev, int32_t nsym, int32_t limit, uint8_t* lengths_dev, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return png_debug_build_code(counts_dev, nsym, limit, lengths_dev, (hipStream_t)stream);
}

size_t resr_fullref_planes_workspace_bytes(const ResrFullRefPlanesDesc* d) { return fullref_planes_workspace_bytes(d); }

int resr_fullref_planes(const ResrFullRefPlanesDesc* d, const void* sr, const void* hr, int64_t* sse, double* psnr, double* ssim, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return fullref_planes_dispatch(d, sr, hr, sse, psnr, ssim, (hipStream_t)stream);
}

int resr_filter2d(const float* src, float* dst, const float* kernel, int32_t n, int32_t c, int32_t h, int32_t w, int32_t kh,
                  int32_t kw, int32_t per_sample, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return filter2d_dispatch(src, dst, kernel, n, c, h, w, kh, kw, per_sample, (hipStream_t)stream);
}

int resr_usm_sharp(const float* src, float* dst, float* tmp3, const float* k1d, int32_t ksize, float weight, float threshold,
                   int32_t n, int32_t c, int32_t h, int32_t w, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return usm_dispatch(src, dst, tmp3, k1d, ksize, weight, threshold, n, c, h, w, (hipStream_t)stream, 1);
}

int resr_usm_sharp_forward_only(const float* src, float* dst, float* tmp3, const float* k1d, int32_t ksize, float weight, float threshold,
                                int32_t n, int32_t c, int32_t h, int32_t w, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return usm_dispatch(src, dst, tmp3, k1d, ksize, weight, threshold, n, c, h, w, (hipStream_t)stream, 0);
}

int resr_usm_sharp_bwd(const float* x, const float* saved_tmp3, const float* g, float* gx, float* tmp2, const float* k1d,
                       int32_t ksize, float weight, int32_t n, int32_t c, int32_t h, int32_t w, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return usm_bwd_dispatch(x, saved_tmp3, g, gx, tmp2, k1d, ksize, weight, n, c, h, w, (hipStream_t)stream);
}

int resr_resize(const float* src, float* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t mode,
                double scale_h, double scale_w, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return resize_dispatch(src, dst, n, c, h, w, oh, ow, mode, scale_h, scale_w, (hipStream_t)stream);
}

int resr_randn_fill(float* dst, int64_t count, uint64_t seed, uint64_t stream_id, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return randn_dispatch(dst, (long)count, seed, stream_id, (hipStream_t)stream);
}

int resr_noise_gaussian(const float* src, float* dst, const float* sigma, const float* gray, const float* field_gray,
                        const float* field_color, int32_t n, int32_t c, int32_t h, int32_t w, int32_t clip, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return gauss_noise_dispatch(src, dst, sigma, gray, field_gray, field_color, n, c, h, w, clip, (hipStream_t)stream);
}

size_t resr_noise_poisson_workspace_bytes(int32_t n) { return (size_t)n * (512 * sizeof(unsigned) + 2 * sizeof(float)); }

int resr_noise_poisson(const float* src, float* dst, const float* scale, const float* gray, uint64_t seed, void* workspace,
                       int32_t n, int32_t c, int32_t h, int32_t w, int32_t clip, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return poisson_noise_dispatch(src, dst, scale, gray, seed, workspace, n, c, h, w, clip, (hipStream_t)stream);
}

int resr_jpeg(const float* src, float* dst, const float* quality, float* coeffs, int32_t n, int32_t h, int32_t w, int32_t flags,
              void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return jpeg_dispatch(src, dst, quality, coeffs, n, h, w, flags, (hipStream_t)stream);
}

int resr_quantize_crop(const float* lr, const float* hr, float* lr_out, float* hr_out, int32_t n, int32_t c, int32_t lr_h,
                       int32_t lr_w, int32_t hr_h, int32_t hr_w, int32_t hr_size, int32_t upscale, int32_t hr_top,
                       int32_t hr_left, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return quantize_crop_dispatch(lr, hr, lr_out, hr_out, n, c, lr_h, lr_w, hr_h, hr_w, hr_size, upscale, hr_top, hr_left,
                                  (hipStream_t)stream);
}

int resr_filter2d_u8(const uint8_t* src, uint8_t* dst, const int32_t* taps_q14, int32_t n, int32_t c, int32_t h, int32_t w,
                     int32_t kh, int32_t kw, int32_t per_sample, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return filter2d_u8_dispatch(src, dst, taps_q14, n, c, h, w, kh, kw, per_sample, (hipStream_t)stream);
}

int resr_resize_u8(const uint8_t* src, uint8_t* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow,
                   int32_t mode, const int32_t* idx_y, const int32_t* w_y, const int32_t* idx_x, const int32_t* w_x, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return resize_u8_dispatch(src, dst, n, c, h, w, oh, ow, mode, idx_y, w_y, idx_x, w_x, (hipStream_t)stream);
}

int resr_jpeg_u8(const uint8_t* src, uint8_t* dst, const float* quality, int32_t* coeffs, int32_t n, int32_t h, int32_t w,
                 void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return jpeg_u8_dispatch(src, dst, quality, coeffs, n, h, w, (hipStream_t)stream);
}

int resr_space_to_depth(const void* src, void* dst, int32_t n, int32_t h, int32_t w, int32_t c, int32_t dtype, int32_t inverse,
                        void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return s2d_dispatch(src, dst, n, h, w, c, dtype, inverse, (hipStream_t)stream);
}

int resr_bilinear_up2x(const void* src, void* dst, int32_t n, int32_t h, int32_t w, int32_t c, int32_t dtype, int32_t backward,
                       void* stream) {
    RESR_DEVICE_SCOPE(stream);
    // RESR_F16X2: src and dst are (hi, lo) pairs, each lo tensor directly behind its hi tensor
    const long px = (long)n * h * w * c;
    const bool x2 = dtype == RESR_F16X2;
    return bilinear_up_dispatch(src, dst, n, h, w, c, dtype, backward, (hipStream_t)stream, x2 ? (backward ? 4 * px : px) : 0L, x2 ? (backward ? px : 4 * px) : 0L);
}

int resr_add_mask(const void* a, const void* b, const void* mask, void* out, int64_t count, int32_t dtype, float slope,
                  void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return add_mask_dispatch(a, b, mask, out, (long)count, dtype, slope, (hipStream_t)stream);
}

int resr_l1_partial(const void* a, const void* b, int64_t count, int32_t dtype, int64_t lo_offset, float* partial, int32_t nblocks, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return l1_partial_dispatch(a, b, (long)count, dtype, (long)lo_offset, partial, nblocks, (hipStream_t)stream);
}

int resr_debug_sustained(int32_t mode, double seconds, const void* src, size_t bytes, void* counter8, double* stream_tbs, double* matrix_pflops,
                         void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return sustained_run(mode, seconds, src, bytes, counter8, stream_tbs, matrix_pflops, (hipStream_t)stream);
}

size_t resr_loss_scratch_bytes(void) { return (1 + 1024) * sizeof(float); }

int resr_bce_logits_const(const float* logits, int64_t count, float label, float weight, float* loss, float* grad, float* scratch,
                          void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return bce_logits_const_dispatch(logits, (long)count, label, weight, loss, grad, scratch, (hipStream_t)stream);
}

int resr_l1_mean(const float* a, const float* b, int64_t count, float weight, float* loss, float* grad_a, float* scratch, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return l1_mean_dispatch(a, b, (long)count, weight, loss, grad_a, scratch, (hipStream_t)stream);
}

int resr_weighted_row_sums(const float* partial, int32_t rows, int32_t cols, const float* coef_host, float* out, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return weighted_rows_dispatch(partial, rows, cols, coef_host, out, (hipStream_t)stream);
}

int resr_spectral_norm(const float* w, float* u, float* v, int32_t rows, int32_t cols, int32_t training, float eps, float* sigma2,
                       float* tmp, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return spectral_norm_dispatch(w, u, v, rows, cols, training, eps, sigma2, tmp, (hipStream_t)stream);
}

int resr_spectral_norm_bwd(const float* g, const float* w, const float* u, const float* v, const float* sigma2, float* dst,
                           int32_t rows, int32_t cols, int32_t accumulate, float* tmp1, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return spectral_norm_bwd_dispatch(g, w, u, v, sigma2, dst, rows, cols, accumulate, tmp1, (hipStream_t)stream);
}

int resr_maxpool2x2(const void* src, void* dst, int32_t n, int32_t h_out, int32_t w_out, int32_t c, int32_t dtype, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    const long px = (long)n * h_out * w_out * c;
    const bool x2 = dtype == RESR_F16X2;
    return maxpool2x2_dispatch(src, dst, n, h_out, w_out, c, dtype, (hipStream_t)stream, x2 ? 4 * px : 0L, x2 ? px : 0L, nullptr);
}

int resr_maxpool2x2_arg(const void* src, void* dst, uint8_t* arg, int32_t n, int32_t h_out, int32_t w_out, int32_t c, int32_t dtype,
                        void* stream) {
    RESR_DEVICE_SCOPE(stream);
    const long px = (long)n * h_out * w_out * c;
    const bool x2 = dtype == RESR_F16X2;
    return maxpool2x2_dispatch(src, dst, n, h_out, w_out, c, dtype, (hipStream_t)stream, x2 ? 4 * px : 0L, x2 ? px : 0L, arg);
}

int resr_maxpool2x2_bwd(const void* g, const uint8_t* arg, void* gin, int32_t n, int32_t h_out, int32_t w_out, int32_t c, int32_t dtype,
                        void* stream) {
    RESR_DEVICE_SCOPE(stream);
    const long px = (long)n * h_out * w_out * c;
    const bool x2 = dtype == RESR_F16X2;
    return maxpool2x2_bwd_dispatch(g, arg, gin, n, h_out, w_out, c, dtype, (hipStream_t)stream, x2 ? px : 0L, x2 ? 4 * px : 0L);
}

int resr_fold4x4(const float* dw3, float* dw4, int32_t cout, int32_t c, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return fold4x4_dispatch(dw3, dw4, cout, c, (hipStream_t)stream);
}

// test entries of the helpers that only the native discriminator passes call (include/resr_debug.h); RESR_F16X2: every lo tensor
// directly behind its hi tensor
int resr_debug_d2s_add_mask(const void* src, const void* add, const void* mask, void* out, int32_t n, int32_t h, int32_t w, int32_t c,
                            int32_t dtype, float slope, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    const long px = dtype == RESR_F16X2 ? (long)n * h * w * c : 0L;   // src [n,h/2,w/2,4c], add and out [n,h,w,c]: the same element count
    return d2s_add_mask_dispatch(src, add, mask, out, n, h, w, c, dtype, slope, (hipStream_t)stream, px, px, px);
}

int resr_debug_bilinear_up2x_bwd_mask(const void* g, void* gin, const void* mask, void* gmasked, int32_t n, int32_t h, int32_t w,
                                      int32_t c, int32_t dtype, float slope, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    const long px = dtype == RESR_F16X2 ? (long)n * h * w * c : 0L;
    return bilinear_up_bwd_mask_dispatch(g, gin, mask, gmasked, n, h, w, c, dtype, slope, (hipStream_t)stream, 4 * px, px);
}

// test entry of nchw_to_nhwc with a prescale slot (tests/test_gpu_pad_skip.py): resr_nchw_to_nhwc passes none
int resr_debug_nchw_to_nhwc(const float* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t unshuffle, int32_t c_pad, int32_t dtype,
                            const uint8_t* mask, const void* amax, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return nchw_to_nhwc_scaled_dispatch(src, dst, n, c, h, w, unshuffle, c_pad, dtype, mask, (hipStream_t)stream, -1L, (const unsigned*)amax);
}

// test entries of the layout kernels as the generator's passes call them (tests/test_gpu_layout_kernels.py): every argument of the
// dispatch function visible, nothing decided here
int resr_debug_absmax(const float* src, int64_t count, void* slot, int32_t target_log2, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return absmax_dispatch(src, (long)count, (unsigned*)slot, target_log2, (hipStream_t)stream);
}

int resr_debug_add_inplace(void* dst, const void* src, int64_t count, int32_t dtype, int64_t dst_lo, int64_t src_lo, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return add_inplace_dispatch(dst, src, (long)count, dtype, (hipStream_t)stream, (long)dst_lo, (long)src_lo);
}

int resr_debug_nchw_to_nhwc_q(const float* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t unshuffle, int32_t c_pad,
                              int32_t dtype, const uint8_t* mask, int64_t lo_off, const void* amax, int64_t q_off, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return nchw_to_nhwc_q_dispatch(src, dst, n, c, h, w, unshuffle, c_pad, dtype, mask, (hipStream_t)stream, (long)lo_off, (const unsigned*)amax,
                                   (long)q_off);
}

int resr_debug_nhwc_to_nchw(const void* src, float* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t shuffle, int32_t src_stride,
                            int32_t dtype, int64_t lo_off, const void* amax, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return nhwc_to_nchw_scaled_dispatch(src, dst, n, c, h, w, shuffle, src_stride, dtype, (hipStream_t)stream, (long)lo_off, (const unsigned*)amax);
}

int resr_debug_sumpool2x2(const void* src, void* dst, const void* mask, int32_t n, int32_t h_out, int32_t w_out, int32_t c, int32_t dtype,
                          float slope, int64_t src_lo, int64_t dst_lo, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return sumpool2x2_dispatch(src, dst, mask, n, h_out, w_out, c, dtype, slope, (hipStream_t)stream, (long)src_lo, (long)dst_lo);
}

// test entry of the compact generator's PReLU pass (tests/test_gpu_kernels.py): the dispatch function compact.hip calls, alone
int resr_debug_conv3x3_prelu(const ResrConvDesc* d, const void* in0, const void* w_packed, const float* bias, const float* prelu,
                             void* out, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    if (!d) return fail(RESR_ERR_ARG, "resr_debug_conv3x3_prelu: null descriptor");
    return conv3x3_dispatch_prelu(d, in0, w_packed, bias, prelu, out, (hipStream_t)stream);
}

// test entries of the compact generator's training kernels (tests/test_gpu_compact_train_kernels.py): the dispatch functions compact.hip calls, alone
int resr_debug_compact_act(const void* z, void* a, const float* slopes, int64_t pixels, int32_t dtype, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_act_dispatch(z, a, slopes, pixels, dtype, (hipStream_t)stream);
}

int resr_debug_compact_act_bwd(const void* g, const void* z, void* gz, const float* slopes, int64_t pixels, int32_t dtype, float* dslope,
                               float* partial, size_t partial_bytes, const void* amax, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_act_bwd_dispatch(g, z, gz, slopes, pixels, dtype, dslope, partial, partial_bytes, (const unsigned*)amax, (hipStream_t)stream);
}

int resr_debug_compact_residual_bwd(const float* gy, float* gx, int32_t n, int32_t h, int32_t w, int32_t s, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return compact_residual_bwd_dispatch(gy, gx, n, h, w, s, (hipStream_t)stream);
}

// test entry (tests/test_gpu_compact_train_passes.py): where the training passes keep their tensors in the workspace; host only
int64_t resr_debug_compact_train_offsets(const ResrCompactDesc* d, int64_t* out, int64_t capacity) {
    return compact_train_offsets(d, out, capacity);
}

// test entry (tests/test_gpu_generator_passes.py): where the RRDB generator's training passes keep their tensors; host only
int64_t resr_debug_generator_train_offsets(const ResrGeneratorDesc* d, int64_t* out, int64_t capacity) {
    return generator_train_offsets(d, out, capacity);
}

// test entry of the resize launch plan (tests/test_resize_surface.py): resize_plan alone.  It only null-checks the tables and looks at
// the alignment of y, so one aligned placeholder stands for all five.
int resr_debug_resize_plan(int32_t n, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t taps_y, int32_t taps_x,
                           int32_t kind, int32_t* plan) {
    alignas(16) static const char placeholder[16] = {};
    if (!plan) return fail(RESR_ERR_ARG, "resr_debug_resize_plan: null argument");
    if (kind < RESIZE_F32 || kind > RESIZE_YUV10) return fail(RESR_ERR_ARG, "resr_debug_resize_plan: kind %d", kind);
    ResizeGeom g;
    const int rc = resize_plan("resr_debug_resize_plan", n, c, h, w, oh, ow, placeholder, placeholder, taps_y, placeholder, placeholder, taps_x,
                               kind, placeholder, &g);
    if (rc) return rc;
    plan[0] = g.th; plan[1] = g.tw; plan[2] = g.rh; plan[3] = g.rw; plan[4] = g.pitch;
    plan[5] = (int32_t)resize_lds_bytes(&g, kind);
    return RESR_OK;
}

// ... and of the image modes' scaled tail (tests/test_image_outscale_surface.py): the tile resr_compact_forward_image_scaled launches
int resr_debug_image_resize_plan(int32_t h, int32_t w, int32_t s, int32_t oh, int32_t ow, int32_t taps_y, int32_t taps_x, int32_t channels,
                                 int32_t bits, int32_t* plan) {
    if (!plan) return fail(RESR_ERR_ARG, "resr_debug_image_resize_plan: null argument");
    ResizeGeom g;
    int kind;
    if (!image_scaled_plan(h, w, s, oh, ow, taps_y, taps_x, channels, bits, &g, &kind))
        return fail(RESR_ERR_ARG, "resr_debug_image_resize_plan: a bad argument, or no tile fits %d x %d taps", taps_y, taps_x);
    plan[0] = g.th; plan[1] = g.tw; plan[2] = g.rh; plan[3] = g.rw; plan[4] = g.pitch;
    plan[5] = (int32_t)resize_lds_bytes(&g, kind);
    return RESR_OK;
}

int resr_debug_spectral_norm_batch(int32_t n, const float* const* w, float* const* u, float* const* v, const int32_t* rows,
                                   const int32_t* cols, int32_t training, float eps, float* const* sigma2, float* const* tmp,
                                   void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return spectral_norm_batch_dispatch(n, w, u, v, rows, cols, training, eps, sigma2, tmp, (hipStream_t)stream);
}

int resr_debug_spectral_norm_bwd_batch(int32_t n, const float* const* g, const float* const* w, const float* const* u,
                                       const float* const* v, const float* const* sigma2, float* const* dst, const int32_t* rows,
                                       const int32_t* cols, float* dot, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return spectral_norm_bwd_batch_dispatch(n, g, w, u, v, sigma2, dst, rows, cols, dot, (hipStream_t)stream);
}

int resr_debug_fold4x4_batch(int32_t n, const float* const* dw3, float* const* dw4, const int32_t* cout, const int32_t* c,
                             void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return fold4x4_batch_dispatch(n, dw3, dw4, cout, c, (hipStream_t)stream);
}

int resr_profile_begin(void) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    for (auto& r : g_prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    g_prof.clear();
    g_prof_on = true;
    return RESR_OK;
}

int64_t resr_profile_end(ResrProfEntry* out, int64_t capacity) {
    g_prof_on = false;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    int64_t n = 0;
    for (auto& r : g_prof) {
        (void)hipEventSynchronize(r.e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.e0, r.e1);
        if (out && n < capacity) { out[n].kernel_id = r.id; out[n].ms = ms; out[n].flop = r.flop; out[n].bytes = r.bytes; }
        ++n;
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    g_prof.clear();
    return n;
}

// host logic probe (no GPU): 2x2 grouping of a weight-gradient launch's products
int resr_debug_wgrad_dense_blocks(int32_t nblocks, const void* const* x_ws, const void* const* g_ws, int32_t n, int32_t h, int32_t w, int32_t splits,
                                  float* partial, size_t partial_bytes, float* dw, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    return wgrad_debug_dense_blocks(nblocks, x_ws, g_ws, n, h, w, splits, partial, partial_bytes, dw, (hipStream_t)stream);
}

int resr_debug_wgrad_plan(const int32_t* cin, const int32_t* cout_pad, int32_t nconv, int32_t* out, int32_t max_jobs) {
    return wgrad_debug_plan(cin, cout_pad, nconv, out, max_jobs);
}

int resr_debug_wgrad_batch_plan(const int32_t* convs, int32_t nconv, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t flags, int32_t splits,
                                int32_t* totals, int32_t* jobs, int32_t* reduce, int32_t* quads, int32_t* quads_mx) {
    return wgrad_debug_batch_plan(convs, nconv, dtype, n, h, w, flags, splits, totals, jobs, reduce, quads, quads_mx);
}

// debug: device buffer of 32*2*64 uint64 receiving s_memrealtime stamps of the next conv launches (null = off)
int resr_debug_conv_trace(void* dev_buf) {
    resr::conv_trace_set(dev_buf);
    return RESR_OK;
}

int64_t resr_chain_errors(void) { return (int64_t)resr::conv3x3_chain_errors(); }

int64_t resr_debug_chain_errors(void) {
    (void)hipDeviceSynchronize();   // test / end-of-run entry: every launch enqueued so far has reported
    return (int64_t)resr::conv3x3_chain_errors();
}

int resr_debug_occupy(int32_t workgroups, int32_t lds_bytes, int32_t micros, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    if (workgroups <= 0 || lds_bytes < 256 || lds_bytes > 160 * 1024 || micros <= 0) return fail(RESR_ERR_ARG, "debug_occupy: bad argument");
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&occupy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    hipLaunchKernelGGL(occupy_kernel, dim3(workgroups), dim3(64), (size_t)lds_bytes, (hipStream_t)stream, (unsigned long long)micros * 100ull, (unsigned*)nullptr);
    RESR_CHECK_LAUNCH("occupy_kernel");
    return RESR_OK;
}

int resr_debug_tr_probe(float* out256, void* stream) {
    RESR_DEVICE_SCOPE(stream);
    hipLaunchKernelGGL(tr_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out256);
    RESR_CHECK_LAUNCH("tr_probe_kernel");
    return RESR_OK;
}

}  // extern "C"
