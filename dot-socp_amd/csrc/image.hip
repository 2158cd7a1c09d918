// Problems given as pictures (include/dotsocp.h: dotsocp_imresize*, dotsocp_image_density): MATLAB's imresize -- bicubic,
// antialiased, separable, uint8 rounded after each pass -- and the densities of the reference's image-based examples, on the
// device.  The header states the semantics once; this file and dot-socp_amd/images.py follow them operation by operation
// (product and sum separately rounded, taps ascending), so uint8 results agree byte for byte and doubles bit for bit.
//
//   k_resize_w        a pass along w: one thread per output (y, x_out), consecutive lanes in y -- every tap is a contiguous
//                     read of a column of the input, every store contiguous; no staging.  uint8 with h % 4 == 0: four
//                     rows per lane, one 32-bit load per tap and one 32-bit store
//   k_resize_h        a pass along h: a workgroup makes `rows` consecutive output rows of IMG_COLS columns; the span of
//                     the input column that those rows' taps touch (smallest .. largest index of the tile, host-computed) is
//                     staged in LDS by contiguous loads (uint8: aligned 32-bit words), the taps are read from LDS
//   k_resize_h_direct the same pass without staging, for tiles whose span does not fit (shrinking by more than ~250)
//   k_gray            three planes -> one (rgb2gray)
//   k_place           uint8 tile -> its place in a double picture (the pad of SINGLE, the quadrants of STITCH4)
//   k_block_sums      the partial sums of 256 consecutive entries in k_map_final's order (advect.hip); launch_report_rows
//                     adds them by k_report_final's tree: the one convention for sums (include/dotsocp.h, "Sums")
//   k_normalise       rho = ((nx ny / sum) rho + lower_bound) / (1 + lower_bound), the sum read from device memory
//
// Everything runs on the null stream of the chosen device between the uploads and the one download; the tap tables are
// built on the host (image_table.h) and read from global memory.
#include <vector>

#include "image_table.h"
#include "solver.h"

namespace dotsocp {

constexpr int IMG_COLS = 4;             // columns of a k_resize_h tile, output columns of a k_resize_w workgroup
constexpr int IMG_ROWS = 64;            // most output rows of a k_resize_h tile
constexpr int IMG_SPAN_MAX = 1024;      // most staged input rows per column (doubles: 32 KiB of LDS with IMG_COLS columns)

struct ResizeTab {
    const double *w;        // [n_out][taps]
    const int *idx;         // [n_out][taps], 0-based
    int taps;
};

__device__ inline unsigned char img_round_u8(double acc) {
    double r = floor(acc);
    if (acc - r >= 0.5) r += 1.0;
    r = r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r);
    return (unsigned char)r;
}

template <typename T> __device__ inline T img_store(double acc);
template <> __device__ inline double img_store<double>(double acc) { return acc; }
template <> __device__ inline unsigned char img_store<unsigned char>(double acc) { return img_round_u8(acc); }

// in: h x w_in x planes, out: h x w_out x planes.  VEC rows per lane (4: uint8 with h % 4 == 0, else 1).
template <typename T, int VEC>
__global__ void __launch_bounds__(64 * IMG_COLS) k_resize_w(const T *__restrict__ in, T *__restrict__ out, i64 h, i64 w_in, i64 w_out,
                                                            ResizeTab tab) {
    const i64 y = ((i64)blockIdx.x * 64 + threadIdx.x) * VEC;
    const i64 xo = (i64)blockIdx.y * IMG_COLS + threadIdx.y;
    if (y >= h || xo >= w_out) return;
    const T *src = in + (i64)blockIdx.z * h * w_in + y;
    T *dst = out + (i64)blockIdx.z * h * w_out + xo * h + y;
    const double *wr = tab.w + xo * tab.taps;
    const int *ir = tab.idx + xo * tab.taps;
    double acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.0;
    for (int k = 0; k < tab.taps; ++k) {
        const double wk = wr[k];
        const T *col = src + (i64)ir[k] * h;
        if (VEC == 4) {
            const unsigned int v = *reinterpret_cast<const unsigned int *>(col);
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] = __dadd_rn(acc[j], __dmul_rn(wk, (double)((v >> (8 * j)) & 0xffu)));
        } else {
            acc[0] = __dadd_rn(acc[0], __dmul_rn(wk, (double)col[0]));
        }
    }
    if (VEC == 4) {
        unsigned int v = 0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) v |= (unsigned int)img_round_u8(acc[j]) << (8 * j);
        *reinterpret_cast<unsigned int *>(dst) = v;
    } else {
        dst[0] = img_store<T>(acc[0]);
    }
}

// in: h_in x w x planes, out: h_out x w x planes.  Workgroup (rows, IMG_COLS): tile blockIdx.x of `rows` output rows, columns
// IMG_COLS * blockIdx.y .., plane blockIdx.z.  tile_lo / tile_span: the input rows [lo, lo + span) the tile's taps touch.
// LDS: IMG_COLS columns of `stride` elements; uint8 columns are staged from the 32-bit word at or below their first byte
// (`in` is 4-byte aligned and its allocation ends at least 3 bytes behind the picture), so element i sits at shift + i.
template <typename T>
__global__ void __launch_bounds__(IMG_ROWS *IMG_COLS) k_resize_h(const T *__restrict__ in, T *__restrict__ out, i64 h_in, i64 h_out, i64 w,
                                                                 ResizeTab tab, const int *__restrict__ tile_lo,
                                                                 const int *__restrict__ tile_span, int stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char img_lds[];
    T *s = reinterpret_cast<T *>(img_lds);
    const int rows = blockDim.x, tid = threadIdx.y * rows + threadIdx.x, nthr = rows * IMG_COLS;
    const int lo = tile_lo[blockIdx.x], span = tile_span[blockIdx.x];
    const i64 x0 = (i64)blockIdx.y * IMG_COLS;
    const i64 plane = (i64)blockIdx.z * h_in * w;
    int shift[IMG_COLS];
#pragma unroll
    for (int c = 0; c < IMG_COLS; ++c) {
        shift[c] = 0;
        if (x0 + c >= w) continue;
        const i64 g0 = plane + (x0 + c) * h_in + lo;
        if (sizeof(T) == 1) {
            const i64 a0 = g0 & ~(i64)3;
            shift[c] = (int)(g0 - a0);
            const int nwords = (shift[c] + span + 3) / 4;
            const unsigned int *src = reinterpret_cast<const unsigned int *>(in + a0);
            unsigned int *d = reinterpret_cast<unsigned int *>(s + (i64)c * stride);
            for (int i = tid; i < nwords; i += nthr) d[i] = src[i];
        } else {
            for (int i = tid; i < span; i += nthr) s[(i64)c * stride + i] = in[g0 + i];
        }
    }
    __syncthreads();
    const i64 yo = (i64)blockIdx.x * rows + threadIdx.x, x = x0 + threadIdx.y;
    if (yo >= h_out || x >= w) return;
    const double *wr = tab.w + yo * tab.taps;
    const int *ir = tab.idx + yo * tab.taps;
    const T *col = s + (i64)threadIdx.y * stride + shift[threadIdx.y] - lo;
    double acc = 0.0;
    for (int k = 0; k < tab.taps; ++k) acc = __dadd_rn(acc, __dmul_rn(wr[k], (double)col[ir[k]]));
    out[(i64)blockIdx.z * h_out * w + x * h_out + yo] = img_store<T>(acc);
}

template <typename T>
__global__ void __launch_bounds__(256) k_resize_h_direct(const T *__restrict__ in, T *__restrict__ out, i64 h_in, i64 h_out, i64 w,
                                                         i64 planes, ResizeTab tab) {
    const i64 n = h_out * w * planes;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const i64 yo = i % h_out, xp = i / h_out;           // xp = x + w * plane
        const double *wr = tab.w + yo * tab.taps;
        const int *ir = tab.idx + yo * tab.taps;
        const T *col = in + xp * h_in;
        double acc = 0.0;
        for (int k = 0; k < tab.taps; ++k) acc = __dadd_rn(acc, __dmul_rn(wr[k], (double)col[ir[k]]));
        out[i] = img_store<T>(acc);
    }
}

// rgb2gray: three planes of n bytes -> one
__global__ void __launch_bounds__(256) k_gray(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, i64 n) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        double acc = __dmul_rn(0.298936021293775, (double)in[i]);
        acc = __dadd_rn(acc, __dmul_rn(0.587043074451121, (double)in[n + i]));
        acc = __dadd_rn(acc, __dmul_rn(0.114020904255103, (double)in[2 * n + i]));
        out[i] = img_round_u8(acc);
    }
}

// dst (H rows per column) [y0 + y, x0 + x] <- src (h x w uint8) as a double, or (255 - v) / 255
__global__ void __launch_bounds__(256) k_place(const unsigned char *__restrict__ src, i64 h, i64 w, double *__restrict__ dst, i64 H,
                                               i64 y0, i64 x0, int reverse) {
    const i64 n = h * w;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const i64 y = i % h, x = i / h;
        const double v = (double)src[i];
        dst[(x0 + x) * H + y0 + y] = reverse ? (255.0 - v) / 255.0 : v;
    }
}

// partials[b] = the sum of entries 256 b .. 256 b + 255 (behind the end: +0.0) in k_map_final's order: the 64 lanes of a
// wavefront by the halving tree of shuffles, then ((w0 + w1) + w2) + w3
__global__ void __launch_bounds__(256) k_block_sums(const double *__restrict__ v, i64 n, double *__restrict__ partials) {
    __shared__ double s_red[4];
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    double s = i < n ? v[i] : 0.0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

__global__ void __launch_bounds__(256) k_normalise(double *__restrict__ rho, i64 n, double cells, const double *__restrict__ sum,
                                                   double lower_bound) {
    const double factor = cells / sum[0], den = 1.0 + lower_bound;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256)
        rho[i] = __ddiv_rn(__dadd_rn(__dmul_rn(factor, rho[i]), lower_bound), den);
}

namespace {

// the current device for the length of a call; every device buffer of the call, released when it ends
struct ImageCall {
    int prev = -1;
    bool switched = false;
    std::vector<void *> bufs;
    ~ImageCall() {
        for (void *b : bufs) dfree(b);
        if (switched && prev >= 0) (void)hipSetDevice(prev);
    }
    int enter(int device) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
            set_error("no HIP device available (libdotsocp has no CPU fallback)");
            return DOTSOCP_ENODEVICE;
        }
        DS_ARG(device >= 0 && device < n, "device ordinal out of range");
        (void)hipGetDevice(&prev);
        DS_HIP(hipSetDevice(device));
        switched = true;
        (void)hipGetLastError();
        return 0;
    }
    // n elements and a tail: uint8 kernels read whole 32-bit words, and the guard bands start on 8-byte boundaries
    // (DOTSOCP_POISON=1 fills the buffers of doubles only: pixels are uploaded whole, tap indices and tile ranges are integers)
    template <class T> int alloc(T **p, i64 n) {
        const i64 bytes = ((i64)sizeof(T) * n + 4 + 7) / 8 * 8;
        unsigned char *raw = nullptr;
        DS_CHECK(dmalloc(&raw, bytes, is_fp_payload<T>::value));
        bufs.push_back(raw);
        *p = reinterpret_cast<T *>(raw);
        return 0;
    }
};

int upload_table(ImageCall &c, i64 n_in, i64 n_out, ResizeTab *tab, std::vector<int> *host_idx) {
    const int P = imresize_max_taps(n_in, n_out);
    std::vector<double> w((size_t)n_out * P);
    std::vector<int> idx((size_t)n_out * P);
    int taps = 0;
    imresize_table(n_in, n_out, w.data(), idx.data(), &taps);
    double *dw = nullptr;
    int *di = nullptr;
    DS_CHECK(c.alloc(&dw, n_out * taps));
    DS_CHECK(c.alloc(&di, n_out * taps));
    DS_HIP(hipMemcpy(dw, w.data(), sizeof(double) * (size_t)n_out * taps, hipMemcpyHostToDevice));
    DS_HIP(hipMemcpy(di, idx.data(), sizeof(int) * (size_t)n_out * taps, hipMemcpyHostToDevice));
    *tab = ResizeTab{dw, di, taps};
    if (host_idx) {
        idx.resize((size_t)n_out * taps);
        host_idx->swap(idx);
    }
    return 0;
}

template <typename T>
int pass_w(ImageCall &c, const T *in, T *out, i64 h, i64 w_in, i64 w_out, i64 planes) {
    ResizeTab tab;
    DS_CHECK(upload_table(c, w_in, w_out, &tab, nullptr));
    const bool vec = sizeof(T) == 1 && h % 4 == 0;
    const i64 lanes = vec ? h / 4 : h;
    dim3 grid((unsigned)((lanes + 63) / 64), (unsigned)((w_out + IMG_COLS - 1) / IMG_COLS), (unsigned)planes), block(64, IMG_COLS);
    auto kernel = vec ? k_resize_w<T, 4> : k_resize_w<T, 1>;
    DS_KLAUNCH(kernel, grid, block, 0, nullptr, in, out, h, w_in, w_out, tab);
    DS_HIP(hipGetLastError());
    return 0;
}

// the input rows that the output rows [r0, r1) touch
void tile_range(const std::vector<int> &idx, int taps, i64 r0, i64 r1, int *lo, int *hi) {
    int a = idx[(size_t)r0 * taps], b = a;
    for (size_t i = (size_t)r0 * taps; i < (size_t)r1 * taps; ++i) {
        a = idx[i] < a ? idx[i] : a;
        b = idx[i] > b ? idx[i] : b;
    }
    *lo = a;
    *hi = b;
}

template <typename T>
int pass_h(ImageCall &c, const T *in, T *out, i64 h_in, i64 h_out, i64 w, i64 planes) {
    ResizeTab tab;
    std::vector<int> idx;
    DS_CHECK(upload_table(c, h_in, h_out, &tab, &idx));
    // the most rows per tile (a power of two) whose widest span still fits the LDS budget
    int rows = IMG_ROWS, span_max = 0;
    std::vector<int> lo, span;
    for (;; rows /= 2) {
        const i64 tiles = (h_out + rows - 1) / rows;
        lo.assign((size_t)tiles, 0);
        span.assign((size_t)tiles, 0);
        span_max = 0;
        for (i64 t = 0; t < tiles; ++t) {
            int a, b;
            tile_range(idx, tab.taps, t * rows, (t + 1) * rows < h_out ? (t + 1) * rows : h_out, &a, &b);
            lo[t] = a;
            span[t] = b - a + 1;
            span_max = span[t] > span_max ? span[t] : span_max;
        }
        if (span_max <= IMG_SPAN_MAX || rows == 1) break;
    }
    if (span_max > IMG_SPAN_MAX) {
        const i64 n = h_out * w * planes;
        DS_KLAUNCH(k_resize_h_direct<T>, dim3((unsigned)launch_blocks(n, 256)), dim3(256), 0, nullptr, in, out, h_in, h_out, w, planes, tab);
        DS_HIP(hipGetLastError());
        return 0;
    }
    const i64 tiles = (i64)lo.size();
    int *d_lo = nullptr, *d_span = nullptr;
    DS_CHECK(c.alloc(&d_lo, tiles));
    DS_CHECK(c.alloc(&d_span, tiles));
    DS_HIP(hipMemcpy(d_lo, lo.data(), sizeof(int) * (size_t)tiles, hipMemcpyHostToDevice));
    DS_HIP(hipMemcpy(d_span, span.data(), sizeof(int) * (size_t)tiles, hipMemcpyHostToDevice));
    // a column of the stage: the span, for uint8 up to 3 bytes in front and whole words; a multiple of 16 bytes
    const int stride = sizeof(T) == 1 ? (span_max + 3 + 3 + 15) / 16 * 16 : (span_max + 1) / 2 * 2;
    const size_t lds = sizeof(T) * (size_t)stride * IMG_COLS;
    dim3 grid((unsigned)tiles, (unsigned)((w + IMG_COLS - 1) / IMG_COLS), (unsigned)planes), block(rows, IMG_COLS);
    DS_KLAUNCH(k_resize_h<T>, grid, block, lds, nullptr, in, out, h_in, h_out, w, tab, (const int *)d_lo, (const int *)d_span, stride);
    DS_HIP(hipGetLastError());
    return 0;
}

// *out (a new buffer of the call) <- imresize(in): the axis with the smaller scale first, on a tie the rows
template <typename T>
int resize_dev(ImageCall &c, const T *in, i64 h_in, i64 w_in, i64 planes, i64 h_out, i64 w_out, T **out) {
    const double sh = (double)h_out / (double)h_in, sw = (double)w_out / (double)w_in;
    T *mid = nullptr;
    DS_CHECK(c.alloc(out, h_out * w_out * planes));
    if (sw < sh) {
        DS_CHECK(c.alloc(&mid, h_in * w_out * planes));
        DS_CHECK(pass_w(c, in, mid, h_in, w_in, w_out, planes));
        DS_CHECK(pass_h(c, (const T *)mid, *out, h_in, h_out, w_out, planes));
    } else {
        DS_CHECK(c.alloc(&mid, h_out * w_in * planes));
        DS_CHECK(pass_h(c, in, mid, h_in, h_out, w_in, planes));
        DS_CHECK(pass_w(c, (const T *)mid, *out, h_out, w_in, w_out, planes));
    }
    return 0;
}

template <typename T>
int imresize_host(ImageCall &c, void *out, const void *in, i64 h_in, i64 w_in, i64 planes, i64 h_out, i64 w_out) {
    T *d_in = nullptr, *d_out = nullptr;
    DS_CHECK(c.alloc(&d_in, h_in * w_in * planes));
    DS_HIP(hipMemcpy(d_in, in, sizeof(T) * (size_t)(h_in * w_in * planes), hipMemcpyHostToDevice));
    DS_CHECK(resize_dev<T>(c, d_in, h_in, w_in, planes, h_out, w_out, &d_out));
    DS_HIP(hipDeviceSynchronize());
    DS_HIP(hipMemcpy(out, d_out, sizeof(T) * (size_t)(h_out * w_out * planes), hipMemcpyDeviceToHost));
    return 0;
}

int gray_dev(ImageCall &c, const unsigned char *in, i64 n, unsigned char **out) {
    DS_CHECK(c.alloc(out, n));
    DS_KLAUNCH(k_gray, dim3((unsigned)launch_blocks(n, 256)), dim3(256), 0, nullptr, in, *out, n);
    DS_HIP(hipGetLastError());
    return 0;
}

int place_dev(const unsigned char *src, i64 h, i64 w, double *dst, i64 H, i64 y0, i64 x0, int reverse) {
    DS_KLAUNCH(k_place, dim3((unsigned)launch_blocks(h * w, 256)), dim3(256), 0, nullptr, src, h, w, dst, H, y0, x0, reverse);
    DS_HIP(hipGetLastError());
    return 0;
}

int upload_image(ImageCall &c, const dotsocp_image &im, unsigned char **d) {
    const i64 n = im.h * im.w * im.planes;
    DS_CHECK(c.alloc(d, n));
    DS_HIP(hipMemcpy(*d, im.pix, (size_t)n, hipMemcpyHostToDevice));
    return 0;
}

}  // namespace

int image_resize(void *out, const void *in, int dtype, i64 h_in, i64 w_in, i64 planes, i64 h_out, i64 w_out, int device) {
    DS_ARG(dtype == DOTSOCP_IMG_U8 || dtype == DOTSOCP_IMG_F64, "imresize: dtype is DOTSOCP_IMG_U8 or DOTSOCP_IMG_F64");
    DS_ARG(imresize_lengths_ok(h_in, h_out) && imresize_lengths_ok(w_in, w_out), "imresize: lengths must lie in 1 .. 65536");
    DS_ARG(planes >= 1 && planes <= 4, "imresize: planes must lie in 1 .. 4");
    DS_ARG(out && in, "imresize: NULL pointer");
    DS_ARG(out != in, "imresize: out and in are the same array");
    ImageCall c;
    DS_CHECK(c.enter(device));
    if (dtype == DOTSOCP_IMG_U8) return imresize_host<unsigned char>(c, out, in, h_in, w_in, planes, h_out, w_out);
    return imresize_host<double>(c, out, in, h_in, w_in, planes, h_out, w_out);
}

int image_density(const dotsocp_image_opts *o, const dotsocp_image *imgs, int nimg, double *rho, int device) {
    DS_ARG(o && imgs && rho, "image_density: NULL pointer");
    DS_ARG(o->layout == DOTSOCP_IMG_SINGLE || o->layout == DOTSOCP_IMG_STITCH4, "image_density: layout is DOTSOCP_IMG_SINGLE or DOTSOCP_IMG_STITCH4");
    DS_ARG(nimg == (o->layout == DOTSOCP_IMG_SINGLE ? 1 : 4), "image_density: SINGLE takes one picture, STITCH4 four");
    DS_ARG(o->ny >= 2 && o->nx >= 2 && o->ny <= IMG_MAX_LEN && o->nx <= IMG_MAX_LEN, "image_density: ny and nx must lie in 2 .. 65536");
    DS_ARG(!(o->reverse && o->layout == DOTSOCP_IMG_STITCH4), "image_density: reverse belongs to DOTSOCP_IMG_SINGLE");
    DS_ARG(std::isfinite(o->lower_bound) && o->lower_bound > -1.0, "image_density: lower_bound must be finite and > -1");
    for (int i = 0; i < nimg; ++i) {
        DS_ARG(imgs[i].pix != nullptr, "image_density: a picture is NULL");
        DS_ARG(imresize_lengths_ok(imgs[i].h, 1) && imresize_lengths_ok(imgs[i].w, 1), "image_density: picture sizes must lie in 1 .. 65536");
        DS_ARG(imgs[i].planes == 1 || imgs[i].planes == 3, "image_density: a picture has 1 or 3 planes");
    }
    ImageCall c;
    DS_CHECK(c.enter(device));
    const i64 ny = o->ny, nx = o->nx, n = ny * nx;
    double *d_rho = nullptr;
    if (o->layout == DOTSOCP_IMG_SINGLE) {
        const dotsocp_image &im = imgs[0];
        unsigned char *d_img = nullptr, *d_small = nullptr;
        DS_CHECK(upload_image(c, im, &d_img));
        DS_CHECK(resize_dev<unsigned char>(c, d_img, im.h, im.w, im.planes, ny - 1, nx - 1, &d_small));
        if (im.planes == 3) {
            const unsigned char *rgb = d_small;
            DS_CHECK(gray_dev(c, rgb, (ny - 1) * (nx - 1), &d_small));
        }
        DS_CHECK(c.alloc(&d_rho, n));
        DS_HIP(hipMemsetAsync(d_rho, 0, sizeof(double) * (size_t)n, nullptr));
        DS_CHECK(place_dev(d_small, ny - 1, nx - 1, d_rho, ny, 0, 0, o->reverse));
    } else {
        const i64 sub_h = nx / 2, sub_w = ny / 2;       // the reference passes nx as the height
        const i64 H = 2 * sub_h, W = 2 * sub_w;
        double *d_big = nullptr;
        DS_CHECK(c.alloc(&d_big, H * W));
        for (int i = 0; i < 4; ++i) {
            const dotsocp_image &im = imgs[i];
            unsigned char *d_img = nullptr, *d_small = nullptr;
            DS_CHECK(upload_image(c, im, &d_img));
            if (im.planes == 3) {
                const unsigned char *rgb = d_img;
                DS_CHECK(gray_dev(c, rgb, im.h * im.w, &d_img));
            }
            DS_CHECK(resize_dev<unsigned char>(c, d_img, im.h, im.w, 1, sub_h, sub_w, &d_small));
            DS_CHECK(place_dev(d_small, sub_h, sub_w, d_big, H, (i / 2) * sub_h, (i % 2) * sub_w, 0));
        }
        if (H != ny || W != nx) DS_CHECK(resize_dev<double>(c, d_big, H, W, 1, ny, nx, &d_rho));
        else d_rho = d_big;
    }
    const i64 blocks = (n + 255) / 256;
    double *d_part = nullptr;
    DS_CHECK(c.alloc(&d_part, blocks + 1));
    DS_KLAUNCH(k_block_sums, dim3((unsigned)blocks), dim3(256), 0, nullptr, (const double *)d_rho, n, d_part);
    DS_HIP(hipGetLastError());
    DS_CHECK(launch_report_rows(d_part, blocks, 1, d_part + blocks, nullptr));
    DS_KLAUNCH(k_normalise, dim3((unsigned)launch_blocks(n, 256)), dim3(256), 0, nullptr, d_rho, n, (double)n, (const double *)(d_part + blocks),
               o->lower_bound);
    DS_HIP(hipGetLastError());
    DS_HIP(hipDeviceSynchronize());
    DS_HIP(hipMemcpy(rho, d_rho, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace dotsocp
