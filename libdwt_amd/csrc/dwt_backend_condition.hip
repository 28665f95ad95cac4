// dwt_backend_condition.hip -- conditioning of row batches (dwt_util_shift21_med_s, dwt_util_center21_s, dwt_util_scale21_s
// and their primitives, src/libdwt.c:25426-26055) on the device, and their C-ABI (include/libdwt_hip.h).  DESIGN.md s16.
//
// Dense device rows of up to N1D_MAX samples take ONE launch (k_cond_lines) where the batch is small enough for that
// kernel to win (use_fused).  Larger batches, longer rows, and every row when option "cond_fused" is 0, take one small
// kernel per operation: median and shift; per centring iteration a centre kernel, a
// displacement into the other of two images and one flag that crosses to the host (did any row move?); min / max and
// the scale.  Host memory and strided device rows are staged into a dense device image first (frame_stage) and take the
// same two routes there.  The small per-row arrays of the interface (info, center, min, max, displ) may each be host or
// device memory.
#include "dwt_backend.h"

#include <climits>

namespace dwtb {

namespace {

constexpr int kCondFusedWaves = 1; // batches of up to this many rounds of workgroups over the 256 CUs take the fused kernel

// the context's conditioning workspace: per row a median, a minimum, a maximum, a centre, a move, a record; one flag
struct Ws {
	float *med, *mn, *mx;
	int *center, *displ, *info, *moved; // moved[0]: the flag; moved[1], moved[2]: the warning counters of the call
};

// the warning counters of this thread's last call still lie in the workspace; read on demand (dwt_hip_rows_warnings)
thread_local bool t_warn_valid = false;

int carve(int n_lines, Ws *w)
{
	const size_t n = align_up(n_lines, 64);
	if (grow(g.cond_ws, n * 4 * 9 + 256))
		return 1;
	char *p = (char *)g.cond_ws.p;
	w->moved = (int *)p; // (at the front, where dwt_hip_rows_warnings finds the counters whatever the batch was)
	p += 256;
	w->med = (float *)p;
	w->mn = w->med + n;
	w->mx = w->mn + n;
	w->center = (int *)(w->mx + n);
	w->displ = w->center + n;
	w->info = w->displ + n;
	HIP_TRY(hipMemsetAsync(w->moved, 0, 12, g.stream));
	t_warn_valid = false;
	return 0;
}

// a per-row array of the interface <-> the workspace; ends synchronised where host memory takes part
int to_caller(void *dst, const void *ws, size_t bytes)
{
	if (!dst || !bytes)
		return 0;
	const bool dev = dwt_hip_is_device_pointer(dst);
	HIP_TRY(hipMemcpyAsync(dst, ws, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, g.stream));
	if (!dev)
		HIP_TRY(hipStreamSynchronize(g.stream));
	return 0;
}

int from_caller(void *ws, const void *src, size_t bytes)
{
	const bool dev = dwt_hip_is_device_pointer(src);
	HIP_TRY(hipMemcpyAsync(ws, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, g.stream));
	if (!dev)
		HIP_TRY(hipStreamSynchronize(g.stream));
	return 0;
}

int check_rows(const void *ptr, size_t line_stride, size_t elem_stride, int n_lines, int size, bool *dev)
{
	if (check_inited())
		return 1;
	if (!ptr)
		return fail("null pointer argument");
	if (n_lines < 0 || size < 1)
		return fail("bad sizes: %d rows of %d samples", n_lines, size);
	if (elem_stride < 4 || elem_stride > INT_MAX || line_stride > (size_t)LONG_MAX / 2 || (n_lines > 1 && line_stride < elem_stride * (size_t)(size - 1) + 4))
		return fail("rows must be apart (line stride %zu, element stride %zu bytes)", line_stride, elem_stride);
	*dev = dwt_hip_is_device_pointer(ptr);
	if (*dev && check_dev_align({ptr}, {(long)line_stride, (long)elem_stride}))
		return 1;
	return 0;
}

// The rows as a dense device image: where they lie (dense device rows), or staged into frame_a.  *staged tells which.
int dense_rows(const void *ptr, bool dev, long ls, long es, int n_lines, int size, Img *A, bool *staged)
{
	if (dev && es == 4) {
		*A = Img{(char *)ptr, n_lines > 1 ? ls : 4l * size, 4};
		*staged = false;
		return 0;
	}
	*staged = true;
	return frame_stage(Frame{(void *)ptr, n_lines > 1 ? ls : es * size, es, 4, size, n_lines, dev}, g.frame_a, A);
}

int copy_rows(char *dst, long dls, const char *src, long sls, int n_lines, int size)
{
	HIP_TRY(hipMemcpy2DAsync(dst, (size_t)dls, src, (size_t)sls, 4 * (size_t)size, (size_t)n_lines, hipMemcpyDeviceToDevice, g.stream));
	return 0;
}

// the per-operation route over the dense device image A, in place (its centring moves go through frame_b and back)
int condition_per_op(unsigned ops, Img A, int n_lines, int N, int max_iters, float lo, float hi, const Ws &w)
{
	if (launched(launch_info_init(w.info, n_lines, g.stream), "condition", "record"))
		return 1;
	if (ops & kCondMedShift) {
		if (launched(launch_rows_median(A.p, A.sx, n_lines, N, w.med, g.stream), "condition", "median") ||
			launched(launch_elem_op(A.p, A.sx, 4, N, n_lines, 2, 0.f, 0.f, w.med, nullptr, nullptr, g.stream), "condition", "shift"))
			return 1;
	}
	if ((ops & kCondCenter) && max_iters > 0) {
		const long pitch = frame_pitch(4, N);
		if (grow(g.frame_b, (size_t)pitch * n_lines))
			return 1;
		Img cur = A, other{(char *)g.frame_b.p, pitch, 4};
		for (int it = 0; it < max_iters; it++) {
			int moved = 0;
			HIP_TRY(hipMemsetAsync(w.moved, 0, 4, g.stream));
			if (launched(launch_rows_center(cur.p, cur.sx, n_lines, N, w.center, w.displ, w.info, w.moved, w.moved + 1, it > 0, g.stream), "condition", "centre"))
				return 1;
			HIP_TRY(hipMemcpyAsync(&moved, w.moved, 4, hipMemcpyDeviceToHost, g.stream));
			HIP_TRY(hipStreamSynchronize(g.stream));
			if (!moved)
				break;
			if (launched(launch_rows_displace(cur.p, cur.sx, other.p, other.sx, n_lines, N, w.displ, 0, 1, g.stream), "condition", "displace"))
				return 1;
			std::swap(cur, other);
		}
		if (cur.p != A.p && copy_rows(A.p, A.sx, cur.p, cur.sx, n_lines, N))
			return 1;
	}
	if (ops & kCondScale) {
		if (launched(launch_rows_minmax(A.p, A.sx, n_lines, N, w.mn, w.mx, g.stream), "condition", "min/max") ||
			launched(launch_elem_op(A.p, A.sx, 4, N, n_lines, 3, lo, hi, w.mn, w.mx, w.info, g.stream), "condition", "scale"))
			return 1;
	}
	return 0;
}

// Which route conditions dense rows of up to N1D_MAX samples: option "cond_fused" 1 / 0 forces the fused kernel / the
// per-operation kernels; otherwise the measured rule.  The fused kernel keeps cond_rows_per_group(N) rows
// per CU in flight and pays one launch; the per-operation route keeps every row in flight and pays some tens of launches
// and one host round trip per centring iteration.
bool use_fused(int n_lines, int size)
{
	if (size > N1D_MAX || g.cond_fused == 0)
		return false;
	if (g.cond_fused > 0)
		return true;
	return (long)n_lines <= (long)kCondFusedWaves * 256 * cond_rows_per_group(size);
}

} // namespace

void cond_forget_warnings() { t_warn_valid = false; }

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_rows_condition(unsigned ops, void *ptr, size_t line_stride, size_t elem_stride, int n_lines, int size, int max_iters, float lo,
	float hi, int *info)
{
	bool dev = false;
	if (check_rows(ptr, line_stride, elem_stride, n_lines, size, &dev))
		return 1;
	if (!ops || (ops & ~7u))
		return fail("bad operation mask 0x%x", ops);
	if ((ops & DWT_HIP_ROWS_SCALE) && !(hi > lo))
		return fail("scaling takes hi > lo (got %g, %g)", (double)lo, (double)hi);
	if (max_iters < 0)
		return fail("bad iteration count %d", max_iters);
	if (n_lines == 0)
		return 0;
	Ws w;
	if (carve(n_lines, &w))
		return 1;
	Img A;
	bool staged = false;
	if (dense_rows(ptr, dev, (long)line_stride, (long)elem_stride, n_lines, size, &A, &staged))
		return 1;
	if (use_fused(n_lines, size)) {
		CondLineArgs a{};
		a.ptr = A.p;
		a.line_stride = A.sx;
		a.n_lines = n_lines;
		a.N = size;
		a.ops = ops;
		a.max_iters = max_iters;
		a.lo = lo;
		a.hi = hi;
		a.info = info ? w.info : nullptr;
		a.warn = w.moved + 1;
		a.vec = A.sx % 16 == 0 && (uintptr_t)A.p % 16 == 0;
		if (launched(launch_cond_lines(a, g.stream), "condition", "line"))
			return 1;
	} else if (condition_per_op(ops, A, n_lines, size, max_iters, lo, hi, w)) {
		return 1;
	}
	if (staged && frame_unpack(Frame{ptr, n_lines > 1 ? (long)line_stride : (long)elem_stride * size, (long)elem_stride, 4, size, n_lines, dev}, A.p, A.sx))
		return 1;
	t_warn_valid = true;
	return to_caller(info, w.info, (size_t)n_lines * 16);
}

int dwt_hip_rows_center_index(const void *ptr, size_t line_stride, size_t elem_stride, int n_lines, int size, int *center)
{
	bool dev = false;
	if (check_rows(ptr, line_stride, elem_stride, n_lines, size, &dev))
		return 1;
	if (!center)
		return fail("null pointer argument");
	if (n_lines == 0)
		return 0;
	Ws w;
	Img A;
	bool staged = false;
	if (carve(n_lines, &w) || dense_rows(ptr, dev, (long)line_stride, (long)elem_stride, n_lines, size, &A, &staged) ||
		launched(launch_rows_center(A.p, A.sx, n_lines, size, w.center, nullptr, nullptr, nullptr, w.moved + 1, 0, g.stream), "condition", "centre"))
		return 1;
	t_warn_valid = true;
	return to_caller(center, w.center, (size_t)n_lines * 4);
}

int dwt_hip_rows_warnings(int *zero_norm, int *no_index)
{
	int c[2] = {0, 0};
	if (!t_warn_valid || !g.cond_ws.p)
		return fail("no dwt_hip_rows_condition / dwt_hip_rows_center_index call precedes on this thread");
	HIP_TRY(hipMemcpyAsync(c, (const int *)g.cond_ws.p + 1, 8, hipMemcpyDeviceToHost, g.stream));
	HIP_TRY(hipStreamSynchronize(g.stream));
	if (zero_norm)
		*zero_norm = c[0];
	if (no_index)
		*no_index = c[1];
	return 0;
}

int dwt_hip_rows_min_max(const void *ptr, size_t line_stride, size_t elem_stride, int n_lines, int size, float *min, float *max)
{
	bool dev = false;
	if (check_rows(ptr, line_stride, elem_stride, n_lines, size, &dev))
		return 1;
	if (!min || !max)
		return fail("null pointer argument");
	if (n_lines == 0)
		return 0;
	Ws w;
	Img A;
	bool staged = false;
	if (carve(n_lines, &w) || dense_rows(ptr, dev, (long)line_stride, (long)elem_stride, n_lines, size, &A, &staged) ||
		launched(launch_rows_minmax(A.p, A.sx, n_lines, size, w.mn, w.mx, g.stream), "condition", "min/max"))
		return 1;
	return to_caller(min, w.mn, (size_t)n_lines * 4) || to_caller(max, w.mx, (size_t)n_lines * 4);
}

int dwt_hip_rows_displace(void *ptr, size_t line_stride, size_t elem_stride, int n_lines, int size, const int *displ, int displ_all,
	int zero_fill)
{
	bool dev = false;
	if (check_rows(ptr, line_stride, elem_stride, n_lines, size, &dev))
		return 1;
	if (n_lines == 0)
		return 0;
	Ws w;
	Img A;
	bool staged = false;
	if (carve(n_lines, &w) || (displ && from_caller(w.displ, displ, (size_t)n_lines * 4)) ||
		dense_rows(ptr, dev, (long)line_stride, (long)elem_stride, n_lines, size, &A, &staged))
		return 1;
	const long pitch = frame_pitch(4, size);
	if (grow(g.frame_b, (size_t)pitch * n_lines))
		return 1;
	char *B = (char *)g.frame_b.p;
	if (launched(launch_rows_displace(A.p, A.sx, B, pitch, n_lines, size, displ ? w.displ : nullptr, displ_all, zero_fill != 0, g.stream), "condition", "displace"))
		return 1;
	if (staged)
		return frame_unpack(Frame{ptr, n_lines > 1 ? (long)line_stride : (long)elem_stride * size, (long)elem_stride, 4, size, n_lines, dev}, B, pitch);
	return copy_rows(A.p, A.sx, B, pitch, n_lines, size);
}

static int elem_op(void *ptr, int stride_x, int stride_y, int size_x, int size_y, int op, float a)
{
	if (check_inited())
		return 1;
	if (!ptr)
		return fail("null pointer argument");
	if (size_x < 0 || size_y < 0)
		return fail("bad sizes: %d x %d", size_x, size_y);
	if (size_x == 0 || size_y == 0)
		return 0;
	if (stride_y < 4)
		return fail("bad strides: %d, %d bytes", stride_x, stride_y);
	if (size_y == 1)
		stride_x = stride_y * size_x; // (one row: its stride is never used)
	if (dwt_hip_is_device_pointer(ptr))
		return check_dev_align({ptr}, {stride_x, stride_y}) ||
			launched(launch_elem_op((char *)ptr, stride_x, stride_y, size_x, size_y, op, a, 0.f, nullptr, nullptr, nullptr, g.stream), "condition", op ? "scale" : "shift");
	const Frame fr{ptr, stride_x, stride_y, 4, size_x, size_y, false};
	Img A;
	if (frame_stage(fr, g.frame_a, &A) ||
		launched(launch_elem_op(A.p, A.sx, 4, size_x, size_y, op, a, 0.f, nullptr, nullptr, nullptr, g.stream), "condition", op ? "scale" : "shift"))
		return 1;
	return frame_unpack(fr, A.p, A.sx);
}

int dwt_hip_shift(void *ptr, int stride_x, int stride_y, int size_x, int size_y, float a) { return elem_op(ptr, stride_x, stride_y, size_x, size_y, 0, a); }

int dwt_hip_scale(void *ptr, int stride_x, int stride_y, int size_x, int size_y, float a) { return elem_op(ptr, stride_x, stride_y, size_x, size_y, 1, a); }

} // extern "C"
#pragma GCC visibility pop
