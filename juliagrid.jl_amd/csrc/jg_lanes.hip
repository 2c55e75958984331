// jg_lanes.hip -- the memory, the captured graphs, the lane I/O, the staging buffer, the verdict wait and the voltage snapshot of the NR and GN handles
// (jg_lanes.hpp).
#include "jg_lanes.hpp"

#include <chrono>
#include <mutex>
#include <string>
#include <thread>

#include "jg_engine.hpp"

namespace jg {

namespace {

// host order [src_rows][rows] (src_rows = 1: one row for every scenario) -> dst [rows][ld]; lanes beyond the batch and beyond src_rows repeat the last row.
// 64 x 64 tiles through LDS: contiguous reads along the row index, contiguous writes along the lanes.  The rows go up as the host holds them (80 KB for one
// row of a 10 000-bus grid; a host-side transposition to [rows][ld] moved 5 MB per array even for one scenario, and 396 MB for one shared column of
// 96 723 measurements) and this kernel spreads them.
__global__ __launch_bounds__(512) void k_lanes_spread(const double* src, double* dst, int rows, int ld, int batch, int src_rows) {
    __shared__ double tile[64][65];
    const int i0 = blockIdx.x * 64, b0 = blockIdx.y * 64;
    for (int r = threadIdx.y; r < 64; r += blockDim.y) {
        const int b = min(min(b0 + r, batch - 1), src_rows - 1), i = i0 + threadIdx.x;
        tile[r][threadIdx.x] = i < rows ? src[(size_t)b * rows + i] : 0.0;
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 64; r += blockDim.y) {
        const int i = i0 + r, b = b0 + threadIdx.x;
        if (i < rows && b < ld) dst[(size_t)i * ld + b] = tile[threadIdx.x][r];
    }
}

// [n][ld] batch-minor -> columns [off, off + n) of a scenario-major record dst [batch][stride]: blockIdx.z = 0 takes vm to off = 0, 1 takes va to off = n (the
// packed result of a batch is V | theta | ... per scenario; stride = n and one z-layer: a plain [batch][n] array).  64 x 64 tiles: a wave reads and writes
// 512 contiguous bytes.
__global__ __launch_bounds__(512) void k_lanes_collect(const double* vm, const double* va, double* dst, int n, int ld, int batch, long long stride) {
    __shared__ double tile[64][65];
    const double* src = blockIdx.z ? va : vm;
    const int off = blockIdx.z ? n : 0;
    const int i0 = blockIdx.x * 64, b0 = blockIdx.y * 64;
    for (int r = threadIdx.y; r < 64; r += blockDim.y) {
        const int i = i0 + r, b = b0 + threadIdx.x;
        tile[r][threadIdx.x] = (i < n && b < ld) ? src[(size_t)i * ld + b] : 0.0;
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 64; r += blockDim.y) {
        const int b = b0 + r, i = i0 + threadIdx.x;
        if (b < batch && i < n) dst[(size_t)b * stride + off + i] = tile[threadIdx.x][r];
    }
}

// The packed result of a batch is a scenario-major record [batch][stride]: V | theta | iterations | status [| objective] per scenario, one buffer for the one
// gather of a sharded run.  V | theta: collect2; the columns behind them:
__global__ void k_pack_tail(const int* iters, const int* status, const double* obj, double* dst, int batch, long long stride, int off) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch) { double* q = dst + (size_t)b * stride + off; q[0] = (double)iters[b]; q[1] = (double)status[b]; if (obj) q[2] = obj[b]; }
}

__global__ void k_add_iter(int* iters, int n) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n) iters[b] += 1;
}

constexpr double POLL_BELOW_US = 800.0;   // a handle whose waits average more than this blocks in hipStreamSynchronize instead
bool poll_enabled() { static const bool on = knob("POLL", 1) != 0; return on; }

}  // namespace

int Graph::begin(hipStream_t st) {
    reset();
    capture_mutex().lock();
    const hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) return 0;
    capture_mutex().unlock();
    return api_fail(2, std::string("hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal): ") + hipGetErrorString(e));
}

int Graph::end(hipStream_t st, int rc) {
    const char* what = "hipStreamEndCapture(st, &g)";
    hipError_t e = hipStreamEndCapture(st, &g);        // whatever the body did: the stream must not stay in capture mode
    if (!rc && e == hipSuccess) { what = "hipGraphInstantiate(&x, g, nullptr, nullptr, 0)"; e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0); }
    if (!rc && e != hipSuccess) rc = api_fail(2, std::string(what) + ": " + hipGetErrorString(e));
    capture_mutex().unlock();
    if (rc) reset();
    return rc;
}

void Graph::reset() {
    if (x) hipGraphExecDestroy(x);
    if (g) hipGraphDestroy(g);
    x = nullptr; g = nullptr;
}

hipError_t Lanes::block(void** p, size_t bytes, const void* src, size_t src_bytes, bool zero) {
    drop(p);
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; return e; }
    if (std::find(dev_.begin(), dev_.end(), p) == dev_.end()) dev_.push_back(p);
    if (zero) e = sync_fill(*p, 0, bytes, stream);
    if (e == hipSuccess && src_bytes) e = sync_copy(*p, src, src_bytes, hipMemcpyHostToDevice, stream);
    return e;
}

hipError_t Lanes::pinned(void** p, size_t bytes) {
    drop(p);
    const hipError_t e = hipHostMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; return e; }
    if (std::find(pinned_.begin(), pinned_.end(), p) == pinned_.end()) pinned_.push_back(p);
    return e;
}

void Lanes::drop(void** p) {                            // (a pointer stays registered: an empty one costs release_all nothing)
    if (!*p) return;
    if (std::find(pinned_.begin(), pinned_.end(), p) != pinned_.end()) hipHostFree(*p); else hipFree(*p);
    *p = nullptr;
}

void Lanes::release_all() {
    for (void** p : dev_) drop(p);
    for (void** p : pinned_) drop(p);
    dev_.clear(); pinned_.clear();
    stage_bytes = 0;
}

hipError_t Lanes::arena(std::initializer_list<Part> parts) {
    size_t bytes = 0, off = 0;
    for (const Part& q : parts) bytes += (q.bytes + 255) / 256 * 256;
    const hipError_t e = block(&d_arena, bytes, nullptr, 0, true);
    if (e != hipSuccess) return e;
    for (const Part& q : parts) { *q.p = (char*)d_arena + off; off += (q.bytes + 255) / 256 * 256; }
    return hipSuccess;
}

int Lanes::upload_fail(hipError_t e) { return e == hipSuccess ? 0 : api_fail(2, std::string("upload: ") + hipGetErrorString(e)); }

void Lanes::collect(const double* src, double* dst, int rows) const {
    hipLaunchKernelGGL(k_lanes_collect, dim3((rows + 63) / 64, ld / 64), dim3(64, 8), 0, stream, src, src, dst, rows, ld, batch, (long long)rows);
}
void Lanes::collect2(const double* a, const double* b, double* dst, int rows, long long stride) const {
    hipLaunchKernelGGL(k_lanes_collect, dim3((rows + 63) / 64, ld / 64, 2), dim3(64, 8), 0, stream, a, b, dst, rows, ld, batch, stride);
}
void Lanes::pack_tail(const int* iters, const int* status, const double* obj, double* dst, long long stride, int off) const {
    hipLaunchKernelGGL(k_pack_tail, dim3((batch + 255) / 256), dim3(256), 0, stream, iters, status, obj, dst, batch, stride, off);
}
void Lanes::add_iter(int* iters) const { hipLaunchKernelGGL(k_add_iter, dim3((ld + 255) / 256), dim3(256), 0, stream, iters, ld); }

// grows only (freeing it after every call would synchronise the device each time -- while another host thread of a pipeline may be capturing its hipGraph);
// a grow frees the old block, after whatever still reads it on the stream has finished
int Lanes::stage_room(size_t bytes) {
    if (bytes <= stage_bytes) return 0;
    JG_API_HIP(hipStreamSynchronize(stream));
    stage_bytes = 0;
    JG_API_HIP(alloc(&d_stage, (bytes + sizeof(double) - 1) / sizeof(double)));
    stage_bytes = bytes;
    return 0;
}

int Lanes::put_rows(double* dst, const double* src, int64_t stride, int rows) {
    if (stride != 0 && stride != rows) {                         // a caller's own row pitch: the general (slow) way
        std::vector<double> t((size_t)rows * ld, 0.0);
        for (int b = 0; b < ld; ++b) {
            const double* s = src + (size_t)(b < batch ? b : batch - 1) * (size_t)stride;   // pad with the last scenario
            for (int i = 0; i < rows; ++i) t[(size_t)i * ld + b] = s[i];
        }
        JG_API_HIP(sync_copy(dst, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        return 0;
    }
    const int src_rows = stride == 0 ? 1 : batch;
    const size_t bytes = (size_t)src_rows * rows * sizeof(double);
    if (int rc = stage_room(bytes)) return rc;
    JG_API_HIP(sync_copy(d_stage, src, bytes, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_lanes_spread, dim3((rows + 63) / 64, ld / 64), dim3(64, 8), 0, stream, (const double*)d_stage, dst, rows, ld, batch, src_rows);
    JG_API_HIP(hipGetLastError());
    JG_API_HIP(hipStreamSynchronize(stream));
    return 0;
}

int Lanes::get_rows(const double* src, double* dst, size_t rows) {  // transposed on the device, then ONE copy of exactly the rows asked for
    const size_t bytes = (size_t)batch * rows * sizeof(double);
    if (int rc = stage_room(bytes)) return rc;
    collect(src, d_stage, (int)rows);
    JG_API_HIP(hipGetLastError());
    JG_API_HIP(sync_copy(dst, d_stage, bytes, hipMemcpyDeviceToHost, stream));
    return 0;
}

int Lanes::get_rows2(const double* src, double* dst, size_t rows) const {
    std::vector<double> t(rows * ld * 2);
    JG_API_HIP(sync_copy(t.data(), src, t.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    for (int b = 0; b < batch; ++b)
        for (size_t r = 0; r < rows; ++r) { dst[((size_t)b * rows + r) * 2] = t[(r * ld + b) * 2]; dst[((size_t)b * rows + r) * 2 + 1] = t[(r * ld + b) * 2 + 1]; }
    return 0;
}

int Lanes::snapshot(const double* a, const double* b, double** a0, double** b0, int rows) {
    if (!*a0) { JG_API_HIP(alloc(a0, (size_t)rows * ld)); JG_API_HIP(alloc(b0, (size_t)rows * ld)); }
    if (int rc = restore(*a0, *b0, a, b, rows)) return rc;
    JG_API_HIP(hipStreamSynchronize(stream));
    return 0;
}

int Lanes::restore(double* a, double* b, const double* a0, const double* b0, int rows) const {
    const size_t bytes = (size_t)rows * ld * 8;
    JG_API_HIP(hipMemcpyAsync(a, a0, bytes, hipMemcpyDeviceToDevice, stream));
    JG_API_HIP(hipMemcpyAsync(b, b0, bytes, hipMemcpyDeviceToDevice, stream));
    return 0;
}

// The verdict kernel of an iteration graph stores into ONE pinned word.  Waiting for it with hipStreamSynchronize costs a wake-up of ~20 us per iteration -- a
// tenth of a single instance's iteration -- so the host ARMS the word (-1) before the launch and polls it (bounded spin, then yields; hipStreamSynchronize
// after 2 s as the safety net).  The next graph is then launched while the tail of the previous one still runs -- stream order keeps them apart.  JG_POLL=0:
// always the synchronise.
void Lanes::arm() const { if (poll_enabled()) *(volatile int*)h_counter = -1; }

hipError_t Lanes::wait(bool whole) {
    const auto t0 = std::chrono::steady_clock::now();
    auto elapsed = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); };
    // Polling pays where an iteration is SHORT (a single instance of the 10k-bus grid: 366 us per iteration; 1.595 ms per solve spinning against 1.656 with the
    // synchronise).  Where it is long -- a 512-lane batch: 1.6 ms, three of them in flight on a thread each; a Gauss-Newton iteration of 96 723 measurements at
    // 512 lanes: 4.4 ms -- the blocking wait is the right one: measured on one box, interleaved, the pipeline loses 7 - 10 % to three spinning / napping host
    // threads (254 - 264k against 282 - 287k NR it/s at the driver's K = 20).  The handle remembers how long its last waits took and picks by that.
    if (!poll_enabled() || (!whole && wait_us > POLL_BELOW_US)) {
        const hipError_t e = hipStreamSynchronize(stream);
        wait_us = 0.5 * wait_us + 0.5 * elapsed();
        return e;
    }
    volatile int* w = (volatile int*)h_counter;
    for (long spins = 0; *w == -1; ++spins) {
        if ((spins & 63) == 63) {
            const double us = elapsed();
            if (us > 2.0e6) return hipStreamSynchronize(stream);             // something is wrong (or very slow): the blocking wait reports it
            if (us > 2.0 * POLL_BELOW_US) std::this_thread::yield();          // longer than anything this branch is meant for (the first wait of a big batch): give the core away between looks
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    if (!whole) wait_us = 0.5 * wait_us + 0.5 * elapsed();
    return hipSuccess;
}

}  // namespace jg
