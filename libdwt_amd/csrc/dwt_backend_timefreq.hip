// dwt_backend_timefreq.hip -- time-frequency planes of line batches (gabor_ft_s / gabor_wt_s / gabor_st_s and their _arg_
// twins, src/gabor.c) and the plane operators on the device, and their C-ABI (include/libdwt_hip.h).
//
// A bank is `bins` complex kernels with their sizes and centres.  It lives in host memory (so banks can be generated and
// queried without a device); its device image -- the conjugated taps, the bin table, the bins by falling size -- is made
// by the first batch call and kept until the bank is freed.
//
// dwt_hip_timefreq_batch on device memory takes ONE kernel launch whatever n_lines, bins and the kernel sizes: k_tf_tiled
// for dense lines and finite taps, k_tf_plain otherwise and under option "timefreq_tiled" = 0.  The plane operators take
// one launch per call.  Host memory takes the staging detour (dwt_backend.h): lines or planes into a dense device image,
// the result spread back plane by plane.
#include "dwt_backend.h"

#include <climits>
#include <cmath>
#include <numeric>

struct dwt_hip_timefreq_bank {
	int bins = 0;
	std::vector<int> size, center;
	std::vector<long> off;   // first tap of each bin
	std::vector<float> taps; // (re, im) as given
	bool finite = true;
	// the device image
	int device = -1;
	void *d_taps = nullptr, *d_bins = nullptr, *d_order = nullptr;
};

namespace dwtb {

namespace {

void bank_drop_device(dwt_hip_timefreq_bank *b)
{
	for (void **p : {&b->d_taps, &b->d_bins, &b->d_order})
		if (*p) {
			hipFree(*p);
			*p = nullptr;
		}
	b->device = -1;
}

int bank_upload(dwt_hip_timefreq_bank *b)
{
	if (b->device == g.device && b->d_taps)
		return 0;
	bank_drop_device(b);
	const size_t n = b->taps.size() / 2;
	std::vector<float> conj(b->taps);
	for (size_t i = 0; i < n; i++)
		conj[2 * i + 1] = -conj[2 * i + 1];
	std::vector<TfBin> bins(b->bins);
	for (int y = 0; y < b->bins; y++)
		bins[y] = TfBin{b->off[y], b->size[y], b->center[y], b->bins - 1 - y, 0};
	std::vector<int> order(b->bins);
	std::iota(order.begin(), order.end(), 0);
	std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return b->size[p] > b->size[q]; });
	HIP_TRY(hipMalloc(&b->d_taps, conj.size() * sizeof(float)));
	HIP_TRY(hipMalloc(&b->d_bins, bins.size() * sizeof(TfBin)));
	HIP_TRY(hipMalloc(&b->d_order, order.size() * sizeof(int)));
	HIP_TRY(hipMemcpy(b->d_taps, conj.data(), conj.size() * sizeof(float), hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(b->d_bins, bins.data(), bins.size() * sizeof(TfBin), hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(b->d_order, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
	b->device = g.device;
	return 0;
}

// device memory on every side; strides that are multiples of 4 bytes
int tf_device(dwt_hip_timefreq_bank *b, const char *src, long ls, long es, int n_lines, int N, int t0, int nt, int out, char *dst,
	long plane_stride, long row_stride, long dst_es)
{
	if (check_dev_align({src, dst}, {es, ls, plane_stride, row_stride, dst_es}) || bank_upload(b))
		return 1;
	TfArgs a{};
	a.src = src;
	a.src_ls = ls;
	a.src_es = es;
	a.n_lines = n_lines;
	a.N = N;
	a.t0 = t0;
	a.nt = nt;
	a.taps = (const float2 *)b->d_taps;
	a.bins = (const TfBin *)b->d_bins;
	a.order = (const int *)b->d_order;
	a.n_bins = b->bins;
	a.out = out;
	a.dst = dst;
	a.plane_stride = plane_stride;
	a.row_stride = row_stride;
	a.dst_es = dst_es;
	if (g.tf_tiled && b->finite && es == 4)
		return launched(launch_tf_tiled(a, g.stream), "timefreq", "tiled");
	return launched(launch_tf_plain(a, g.stream), "timefreq", "plain");
}

// host or device memory (both sides alike): the checks of the C-ABI entries.  Outputs t0 .. t0+nt-1 of every line.
int timefreq(dwt_hip_timefreq_bank *b, const void *src, long ls, long es, int n_lines, int N, int t0, int nt, int out, void *dst,
	long plane_stride, long row_stride, long dst_es)
{
	if (!b)
		return fail("timefreq: null bank");
	if (out < 0 || out > 2)
		return fail("timefreq: out_kind %d (0: complex, 1: magnitude, 2: argument)", out);
	const int osz = out == kTfComplex ? 8 : 4;
	if (n_lines < 1 || N < 1 || nt < 1 || t0 < 0 || (long)t0 + nt > N)
		return fail("timefreq: bad arguments (%d lines of %d samples; at least one of each)", n_lines, N);
	if (!src || !dst)
		return fail("null pointer argument");
	if (es < 4 || dst_es < osz || ls < 0 || plane_stride < 0 || row_stride < 0)
		return fail("timefreq: bad strides");
	if (n_lines > 1 && ls < es * (long)N)
		return fail("timefreq: lines must be apart (line stride %ld bytes, %d samples)", ls, N);
	const long row_bytes = (nt - 1l) * dst_es + osz, rows_bytes = (b->bins - 1l) * row_stride + row_bytes;
	if (b->bins > 1 && row_stride < row_bytes)
		return fail("timefreq: plane rows must be apart (row stride %ld bytes)", row_stride);
	if (n_lines > 1 && plane_stride < rows_bytes)
		return fail("timefreq: planes must be apart (plane stride %ld bytes)", plane_stride);
	const size_t src_n = (size_t)((n_lines - 1l) * ls + (N - 1l) * es + 4), dst_n = (size_t)((n_lines - 1l) * plane_stride + rows_bytes);
	if (overlap(src, src_n, dst, dst_n))
		return fail("timefreq: src and dst must not overlap");
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(src);
	if (dev != (bool)dwt_hip_is_device_pointer(dst))
		return fail("src and dst must both be host or both be device pointers");
	if (dev)
		return tf_device(b, (const char *)src, ls, es, n_lines, N, t0, nt, out, (char *)dst, plane_stride, row_stride, dst_es);

	// host memory: a dense device image of the lines, dense device planes, each plane spread back
	const Frame fs{(void *)src, ls, es, 4, N, n_lines, false};
	const Frame fd{dst, row_stride, dst_es, osz, nt, b->bins, false};
	if (frame_check(fs) || frame_check(fd))
		return 1;
	const long dpitch = frame_pitch(osz, nt), plane = dpitch * b->bins;
	Img A;
	if (grow(g.frame_b, (size_t)plane * n_lines) || frame_stage(fs, g.frame_a, &A) ||
		tf_device(b, A.p, A.sx, 4, n_lines, N, t0, nt, out, (char *)g.frame_b.p, plane, dpitch, osz))
		return 1;
	return frame_unpack_stack(fd, n_lines, plane_stride, g.frame_b.p, dpitch);
}

// op 0: phase derivative, 1 .. 3: the ridge detectors; element (y, x) of plane p at base + p*ps + y*sx + x*sy on both sides
int plane_op(int op, const void *src, void *dst, long sx, long sy, int size_x, int size_y, int n_planes, long ps, float param, const char *who)
{
	if (size_x < 1 || size_y < 1 || n_planes < 1)
		return fail("%s: bad sizes (%d planes of %d x %d)", who, n_planes, size_x, size_y);
	if (!src || !dst)
		return fail("null pointer argument");
	if (op == 0 && !(param > 0.f))
		return fail("%s: the limit must be positive", who);
	if (sy < 4 || sx < 0 || ps < 0 || (size_y > 1 && sx < sy * (long)size_x))
		return fail("%s: bad strides", who);
	const long plane_bytes = (size_y - 1l) * sx + (size_x - 1l) * sy + 4;
	if (n_planes > 1 && ps < plane_bytes)
		return fail("%s: planes must be apart (plane stride %ld bytes)", who, ps);
	const size_t n = (size_t)((n_planes - 1l) * ps + plane_bytes);
	if (overlap(src, n, dst, n))
		return fail("%s: source and destination must not overlap", who);
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(src);
	if (dev != (bool)dwt_hip_is_device_pointer(dst))
		return fail("source and destination must both be host or both be device pointers");
	TfPlaneArgs a{(const char *)src, (char *)dst, ps, sx, sy, size_x, size_y, n_planes, op, param};
	if (dev) {
		return check_dev_align({src, dst}, {sx, sy, ps}) || launched(launch_tf_plane_op(a, g.stream), "timefreq", who);
	}
	const Frame fs{(void *)src, sx, sy, 4, size_x, size_y, false}, fd{dst, sx, sy, 4, size_x, size_y, false};
	if (frame_check(fs) || frame_check(fd))
		return 1;
	const long pitch = frame_pitch(4, size_x), plane = pitch * size_y;
	if (grow(g.frame_a, (size_t)plane * n_planes) || grow(g.frame_b, (size_t)plane * n_planes) ||
		frame_pack_stack(fs, n_planes, ps, g.frame_a.p, pitch))
		return 1;
	a.src = (const char *)g.frame_a.p;
	a.dst = (char *)g.frame_b.p;
	a.ps = plane;
	a.sx = pitch;
	a.sy = 4;
	return launched(launch_tf_plane_op(a, g.stream), "timefreq", who) || frame_unpack_stack(fd, n_planes, ps, g.frame_b.p, pitch);
}

bool strides_ok(size_t a, size_t b, size_t c, size_t d)
{
	return a <= (size_t)LONG_MAX / 2 && b <= (size_t)LONG_MAX / 2 && c <= (size_t)LONG_MAX / 2 && d <= INT_MAX;
}

} // namespace

} // namespace dwtb

using namespace dwtb;

extern "C" long dwt_tf_generate(int kind, int bins, float sigma, float freq, int *sizes, int *centers, float *taps); // dwt_entry_timefreq.c

#pragma GCC visibility push(default)
extern "C" {

dwt_hip_timefreq_bank *dwt_hip_timefreq_bank_create(int kind, int bins, float sigma, float freq)
{
	if (kind < DWT_HIP_TIMEFREQ_FT || kind > DWT_HIP_TIMEFREQ_ST || bins < 1) {
		fail("timefreq bank: kind %d (0: FT, 1: WT, 2: ST) with %d bins (at least 1)", kind, bins);
		return nullptr;
	}
	if ((kind != DWT_HIP_TIMEFREQ_ST && !(sigma > 0.f)) || (kind == DWT_HIP_TIMEFREQ_WT && !(freq > 0.f))) {
		fail("timefreq bank: sigma %g and frequency %g must be positive", (double)sigma, (double)freq);
		return nullptr;
	}
	std::vector<int> sizes(bins), centers(bins);
	const long total = dwt_tf_generate(kind, bins, sigma, freq, sizes.data(), centers.data(), nullptr);
	if (total < 0) {
		fail("timefreq bank: sigma %g and frequency %g give a kernel size that is no positive int", (double)sigma, (double)freq);
		return nullptr;
	}
	std::vector<float> taps(2 * (size_t)total);
	dwt_tf_generate(kind, bins, sigma, freq, sizes.data(), centers.data(), taps.data());
	return dwt_hip_timefreq_bank_from_kernels(bins, sizes.data(), centers.data(), taps.data());
}

dwt_hip_timefreq_bank *dwt_hip_timefreq_bank_from_kernels(int bins, const int *sizes, const int *centers, const float *taps)
{
	if (bins < 1 || !sizes || !centers || !taps) {
		fail("timefreq bank: %d bins (at least 1), sizes, centres and taps", bins);
		return nullptr;
	}
	long total = 0;
	for (int y = 0; y < bins; y++) {
		if (sizes[y] < 1 || centers[y] < 0 || centers[y] >= sizes[y]) {
			fail("timefreq bank: kernel %d has %d taps and centre %d (0 <= centre < taps)", y, sizes[y], centers[y]);
			return nullptr;
		}
		total += sizes[y];
	}
	dwt_hip_timefreq_bank *b = new dwt_hip_timefreq_bank;
	b->bins = bins;
	b->size.assign(sizes, sizes + bins);
	b->center.assign(centers, centers + bins);
	b->off.resize(bins);
	for (long y = 0, o = 0; y < bins; o += sizes[y++])
		b->off[y] = o;
	b->taps.assign(taps, taps + 2 * total);
	for (float v : b->taps)
		b->finite = b->finite && std::isfinite(v);
	return b;
}

void dwt_hip_timefreq_bank_free(dwt_hip_timefreq_bank *bank)
{
	if (!bank)
		return;
	bank_drop_device(bank);
	delete bank;
}

int dwt_hip_timefreq_bank_bins(const dwt_hip_timefreq_bank *bank) { return bank ? bank->bins : 0; }

long dwt_hip_timefreq_bank_taps(const dwt_hip_timefreq_bank *bank) { return bank ? (long)(bank->taps.size() / 2) : 0; }

int dwt_hip_timefreq_bank_query(const dwt_hip_timefreq_bank *bank, int *sizes, int *centers, float *taps)
{
	if (!bank)
		return fail("timefreq: null bank");
	if (sizes)
		std::copy(bank->size.begin(), bank->size.end(), sizes);
	if (centers)
		std::copy(bank->center.begin(), bank->center.end(), centers);
	if (taps)
		std::copy(bank->taps.begin(), bank->taps.end(), taps);
	return 0;
}

int dwt_hip_timefreq_batch_strided(dwt_hip_timefreq_bank *bank, const void *src, size_t line_stride, size_t elem_stride, int n_lines, int N,
	int out_kind, void *dst, size_t plane_stride, size_t row_stride, size_t dst_elem_stride)
{
	if (!strides_ok(line_stride, plane_stride, row_stride, elem_stride) || dst_elem_stride > INT_MAX)
		return fail("timefreq: bad strides");
	return timefreq(bank, src, (long)line_stride, (long)elem_stride, n_lines, N, 0, N, out_kind, dst, (long)plane_stride, (long)row_stride,
		(long)dst_elem_stride);
}

int dwt_hip_timefreq_batch(dwt_hip_timefreq_bank *bank, const void *src, size_t line_stride, size_t elem_stride, int n_lines, int N,
	int out_kind, void *dst, size_t plane_stride, size_t row_stride)
{
	return dwt_hip_timefreq_batch_strided(bank, src, line_stride, elem_stride, n_lines, N, out_kind, dst, plane_stride, row_stride,
		out_kind == kTfComplex ? 8 : 4);
}

int dwt_hip_gabor_transform(int kind, int arg, const float *sig, int sig_stride, int sig_size, void *plane, int stride_x, int stride_y,
	int bins, float sigma, float freq)
{
	if (sig_stride < 0 || stride_x < 0 || stride_y < 0 || sig_size < 1)
		return fail("timefreq: bad arguments (%d samples, strides %d, %d and %d)", sig_size, sig_stride, stride_x, stride_y);
	dwt_hip_timefreq_bank *bank = dwt_hip_timefreq_bank_create(kind, bins, sigma, freq);
	if (!bank)
		return 1;
	const int rc = timefreq(bank, sig, (long)sig_stride * sig_size, sig_stride, 1, sig_size, 0, sig_size, arg ? kTfArg : kTfAbs, plane,
		(long)stride_x * bins, stride_x, stride_y);
	dwt_hip_timefreq_bank_free(bank);
	return rc;
}

int dwt_hip_timefreq_line(int arg, float *dst, int dst_stride, const float *src, int src_stride, int size, const void *kern, int kern_stride,
	int kern_size, int kern_center)
{
	if (dst_stride < 0 || src_stride < 0 || size < 1 || kern_stride < 8 || kern_size < 1 || !kern)
		return fail("timefreq line: bad arguments (%d samples, %d taps, strides %d, %d and %d)", size, kern_size, dst_stride, src_stride, kern_stride);
	if (dwt_hip_is_device_pointer(kern))
		return fail("timefreq line: the kernel is host memory");
	std::vector<float> taps(2 * (size_t)kern_size);
	for (int i = 0; i < kern_size; i++)
		memcpy(&taps[2 * (size_t)i], (const char *)kern + (size_t)i * kern_stride, 8);
	dwt_hip_timefreq_bank *bank = dwt_hip_timefreq_bank_from_kernels(1, &kern_size, &kern_center, taps.data());
	if (!bank)
		return 1;
	const long row = (long)dst_stride * size;
	const int rc = timefreq(bank, src, (long)src_stride * size, src_stride, 1, size, 0, size, arg ? kTfArg : kTfAbs, dst, row, row, dst_stride);
	dwt_hip_timefreq_bank_free(bank);
	return rc;
}

int dwt_hip_cdot1(const float *func, int func_size, int func_stride, int func_center, const float *kern, int kern_size, int kern_stride,
	int kern_center, float *re_im)
{
	if (!func || !kern || !re_im)
		return fail("null pointer argument");
	if (func_size < 1 || func_center < 0 || func_center >= func_size || func_stride < 4 || kern_stride < 8 || kern_size < 1)
		return fail("cdot1: bad arguments (signal of %d samples, centre %d; kernel of %d taps)", func_size, func_center, kern_size);
	if (dwt_hip_is_device_pointer(kern) || dwt_hip_is_device_pointer(re_im))
		return fail("cdot1: the kernel and the result are host memory");
	std::vector<float> taps(2 * (size_t)kern_size);
	for (int i = 0; i < kern_size; i++)
		memcpy(&taps[2 * (size_t)i], (const char *)kern + (size_t)i * kern_stride, 8);
	dwt_hip_timefreq_bank *b = dwt_hip_timefreq_bank_from_kernels(1, &kern_size, &kern_center, taps.data());
	if (!b)
		return 1;
	// one output, computed where the signal lies; a device signal's result comes back through a staging word pair
	int rc;
	if (dwt_hip_is_device_pointer(func)) {
		rc = check_inited() || grow(g.frame_b, 8) ||
			timefreq(b, func, (long)func_stride * func_size, func_stride, 1, func_size, func_center, 1, kTfComplex, g.frame_b.p, 8, 8, 8);
		if (!rc && (hipMemcpyAsync(re_im, g.frame_b.p, 8, hipMemcpyDeviceToHost, g.stream) != hipSuccess || hipStreamSynchronize(g.stream) != hipSuccess))
			rc = fail("cdot1: the result could not be read back");
	} else
		rc = timefreq(b, func, (long)func_stride * func_size, func_stride, 1, func_size, func_center, 1, kTfComplex, re_im, 8, 8, 8);
	dwt_hip_timefreq_bank_free(b);
	return rc;
}

int dwt_hip_phase_derivative(const void *angle, void *derivative, int stride_x, int stride_y, int size_x, int size_y, int n_planes,
	size_t plane_stride, float limit)
{
	if (plane_stride > (size_t)LONG_MAX / 2)
		return fail("phase derivative: bad strides");
	return plane_op(0, angle, derivative, stride_x, stride_y, size_x, size_y, n_planes, (long)plane_stride, limit, "phase derivative");
}

int dwt_hip_detect_ridges(int kind, const void *src, void *ridges, int stride_x, int stride_y, int size_x, int size_y, int n_planes,
	size_t plane_stride, float threshold)
{
	if (kind < 1 || kind > 3)
		return fail("detect ridges: kind %d (1: sign change of the magnitude's slope, 2: negative phase derivative, 3: gradient maximum)", kind);
	if (plane_stride > (size_t)LONG_MAX / 2)
		return fail("detect ridges: bad strides");
	return plane_op(kind, src, ridges, stride_x, stride_y, size_x, size_y, n_planes, (long)plane_stride, threshold, "detect ridges");
}

} // extern "C"
#pragma GCC visibility pop
