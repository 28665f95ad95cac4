// dwt_backend_eaw.hip -- the edge-avoiding drivers on the device and their C-ABI (include/libdwt_hip.h): 5/3
// (dwt_eaw53_2f_s / _2i_s, src/libdwt.c:16663, 18373; the interleaved dwt_eaw53_2f_inplace_s / _2i_inplace_s, :16602,
// :17932) and 9/7 (dwt_eaw97_2f_s / _2i_s, src/eaw-experimental.c:300, 398, Mallat only).  The two wavelets' drivers are
// the same loop over different line functions, so one set of functions here takes the wavelet in its frame.
//
// A dense Mallat frame in HBM runs one launch of the wavelet's forward / inverse tile kernel per level (dwt_eaw.hip),
// for a whole batch at once: the level reads a copy of the image (forward level 0, every inverse
// level's detail bands) or the LL ping-pong, so no tile reads what another one writes.  Levels whose LL side has shrunk
// to 1 (decompose_one), sparse frames, the interleaved layout and option "eaw_two_pass" run the reference's loop: per
// level an exact row pass and an exact column pass (each one line kernel into a dense scratch and one placing kernel),
// then its zero fills.  Host memory and strided device images are packed into a dense device image first, as the other
// drivers do.
#include "dwt_backend.h"

#include <climits>

namespace dwtb {

namespace {

struct EawFrame {
	EawWavelet wavelet;
	int layout; // DWT_HIP_EAW_MALLAT / DWT_HIP_EAW_INTERLEAVED
	Geom ge;
	int J;
	long offH[33], offV[33];
	long total; // floats of one image's weights
};

void eaw_layout(EawFrame *f)
{
	long at = 0;
	for (int j = 0; j < f->J; j++) {
		const Geom &ge = f->ge;
		const long nh = f->layout == DWT_HIP_EAW_MALLAT ? (long)ge.Ho(j) * ge.Wi(j) : (long)ge.Hi(j) * ge.Wi(j);
		const long nv = f->layout == DWT_HIP_EAW_MALLAT ? (long)ge.Wo(j) * ge.Hi(j) : (long)ge.Wi(j) * ge.Hi(j);
		f->offH[j] = at;
		at += nh;
		f->offV[j] = at;
		at += nv;
	}
	f->total = at;
}

// the reference's level count: forward clamps *jp (and stores it), inverse takes j_max when 0 <= j_max < limit
int eaw_levels(bool inverse, const Geom &ge, int decompose_one, int *jp)
{
	const int n = decompose_one ? std::max(ge.sox, ge.soy) : std::min(ge.sox, ge.soy);
	const int lim = n == 0 ? 32 : ceil_log2(n); // src/inline.h:443 gives 32 levels of nothing to an empty frame
	if (!inverse) {
		if (*jp < 0 || *jp > lim)
			*jp = lim;
		return *jp;
	}
	return (*jp >= 0 && *jp < lim) ? *jp : lim;
}

// One exact pass over n_lines lines of N samples (dwt_eaw53_{f,i}_ex_stride_s / dwt_eaw97_{f,i}_ex_stride_s on each):
// line kernel into the dense scratch, then the placing kernel.  hoff: Mallat H offset, or -1 for the interleaved layout.
int line_pass(EawWavelet wv, bool inverse, char *base, long ls, long es, int n_lines, int N, int hoff, float *w, float alpha)
{
	if (n_lines <= 0 || N <= 0)
		return 0;
	if (grow(g.frame_b, (size_t)n_lines * N * 4))
		return 1;
	float *tmp = (float *)g.frame_b.p;
	const bool lanes_along_lines = ls < es; // columns of a row-major image
	return launched(launch_eaw_line(wv, inverse, base, ls, es, n_lines, N, hoff, tmp, w, lanes_along_lines, alpha, g.stream), "EAW", "line pass") ||
	       launched(launch_eaw_place(base, ls, es, n_lines, N, inverse ? -1 : hoff, tmp, lanes_along_lines, g.stream), "EAW", "line pass");
}

// Level j of the reference's loop on the dense device image d (4-byte elements, pitch d.sx).
int level_two_pass(bool inverse, const EawFrame &f, Img d, int j, int zero_padding, float *wb, float alpha)
{
	const Geom &ge = f.ge;
	char *p = d.p;
	const long P = d.sx;
	if (f.layout == DWT_HIP_EAW_INTERLEAVED) { // lattice of stride 2^j over the inner frame; zero_padding unused
		const int k = inverse ? j - 1 : j, Wk = ge.Wi(k), Hk = ge.Hi(k);
		const long rs = P << k, cs = 4l << k;
		if (!inverse)
			return line_pass(f.wavelet, false, p, rs, cs, Hk, Wk, -1, wb + f.offH[k], alpha) || line_pass(f.wavelet, false, p, cs, rs, Wk, Hk, -1, wb + f.offV[k], alpha);
		return line_pass(f.wavelet, true, p, cs, rs, Wk, Hk, -1, wb + f.offV[k], alpha) || line_pass(f.wavelet, true, p, rs, cs, Hk, Wk, -1, wb + f.offH[k], alpha);
	}
	if (!inverse) {
		// rows y < size_o_src_y over size_i_src_x samples, then columns x < size_o_src_x over size_i_src_y
		if (line_pass(f.wavelet, false, p, P, 4, ge.Ho(j), ge.Wi(j), ge.Wo(j + 1), wb + f.offH[j], alpha) ||
			line_pass(f.wavelet, false, p, 4, P, ge.Wo(j), ge.Hi(j), ge.Ho(j + 1), wb + f.offV[j], alpha))
			return 1;
		if (zero_padding) { // dwt_zero_padding_f_stride_s (src/libdwt.c:12118), rows then columns
			const int nlx = (ge.Wi(j) + 1) >> 1, nhx = ge.Wi(j) >> 1, nly = (ge.Hi(j) + 1) >> 1, nhy = ge.Hi(j) >> 1;
			if (zero_rect(d, nlx, 0, ge.Wo(j + 1) - nlx, ge.Ho(j)) ||
				zero_rect(d, ge.Wo(j + 1) + nhx, 0, (ge.Wo(j) - ge.Wo(j + 1)) - nhx, ge.Ho(j)) ||
				zero_rect(d, 0, nly, ge.Wo(j), ge.Ho(j + 1) - nly) ||
				zero_rect(d, 0, ge.Ho(j + 1) + nhy, ge.Wo(j), (ge.Ho(j) - ge.Ho(j + 1)) - nhy))
				return 1;
		}
		return 0;
	}
	// level j back to j-1: columns x < size_o_dst_x over size_i_dst_y samples, then rows y < size_o_dst_y
	if (line_pass(f.wavelet, true, p, 4, P, ge.Wo(j - 1), ge.Hi(j - 1), ge.Ho(j), wb + f.offV[j - 1], alpha) ||
		line_pass(f.wavelet, true, p, P, 4, ge.Ho(j - 1), ge.Wi(j - 1), ge.Wo(j), wb + f.offH[j - 1], alpha))
		return 1;
	if (zero_padding) // dwt_zero_padding_i_stride_s (src/libdwt.c:12199), rows then columns
		return zero_rect(d, ge.Wi(j - 1), 0, ge.Wo(j - 1) - ge.Wi(j - 1), ge.Ho(j - 1)) ||
		       zero_rect(d, 0, ge.Hi(j - 1), ge.Wo(j - 1), ge.Ho(j - 1) - ge.Hi(j - 1));
	return 0;
}

bool eaw_fused_ok(const EawFrame &f)
{
	return f.layout == DWT_HIP_EAW_MALLAT && f.ge.dense() && !g.eaw_two_pass;
}

// levels 0 .. n-1 have both sides >= 2 (the fused levels); the deeper ones (decompose_one) run as line passes
int fused_levels(const EawFrame &f)
{
	int n = 0;
	while (n < f.J && f.ge.Wo(n) >= 2 && f.ge.Ho(n) >= 2)
		n++;
	return n;
}

int level_launch(EawWavelet wv, bool inverse, const EawLevelArgs &a, float alpha)
{
	return launched(launch_eaw_level(wv, inverse, a, alpha, g.stream), "EAW", "level");
}

// scratch of the fused levels for the `batch` images at d.p + b*bs: a dense copy of them (frame_b), made here, and the
// LL ping-pong
int fused_scratch(const EawFrame &f, Img d, int batch, long bs, float **copy, float **ll)
{
	const Geom &ge = f.ge;
	const int W = ge.sox, H = ge.soy;
	const size_t img = (size_t)W * H * 4 * batch, llb = (size_t)ge.Wo(1) * ge.Ho(1) * 4 * batch;
	if (grow(g.frame_b, img) || grow(g.eaw_ll[0], llb) || grow(g.eaw_ll[1], llb))
		return 1;
	*copy = (float *)g.frame_b.p;
	ll[0] = (float *)g.eaw_ll[0].p;
	ll[1] = (float *)g.eaw_ll[1].p;
	for (int b = 0; b < batch; b++)
		HIP_TRY(hipMemcpy2DAsync(*copy + (long)b * W * H, (size_t)W * 4, d.p + b * bs, d.sx, (size_t)W * 4, H, hipMemcpyDeviceToDevice, g.stream));
	return 0;
}

// `batch` dense images at d.p + b*bs bytes (pitch d.sx), weights of image b at wb + b*ws floats
int run_device(bool inverse, const EawFrame &f, Img d, int batch, long bs, float *wb, long ws, int zero_padding, float alpha)
{
	const Geom &ge = f.ge;
	const int J = f.J;
	const int nf = eaw_fused_ok(f) ? fused_levels(f) : 0;
	auto two_pass = [&](int j) {
		for (int b = 0; b < batch; b++)
			if (level_two_pass(inverse, f, Img{d.p + b * bs, d.sx, 4}, j, zero_padding, wb + b * ws, alpha))
				return 1;
		return 0;
	};
	// the fused levels: the image copy C (pitch W) and the LL ping-pong (pitch pll), images bll floats apart
	float *C = nullptr, *LL[2] = {nullptr, nullptr};
	const int W = ge.sox, H = ge.soy;
	const long pll = ge.Wo(1), bll = (long)ge.Wo(1) * ge.Ho(1);
	if (!inverse) {
		if (nf > 0) {
			if (fused_scratch(f, d, batch, bs, &C, LL))
				return 1;
			for (int j = 0; j < nf; j++) {
				EawLevelArgs a;
				a.W = ge.Wo(j);
				a.H = ge.Ho(j);
				a.batch = batch;
				a.in = j == 0 ? C : LL[(j - 1) & 1];
				a.pin = j == 0 ? W : pll;
				a.bi_in = j == 0 ? (long)W * H : bll;
				a.det_out = (float *)d.p;
				a.pd = d.sx / 4;
				a.bi_det = bs / 4;
				if (j == nf - 1) { // the last fused level's LL goes home
					a.ll_out = (float *)d.p;
					a.pll = d.sx / 4;
					a.bi_ll = bs / 4;
				} else {
					a.ll_out = LL[j & 1];
					a.pll = pll;
					a.bi_ll = bll;
				}
				a.wH_out = wb + f.offH[j];
				a.wV_out = wb + f.offV[j];
				a.bi_w = ws;
				if (level_launch(f.wavelet, false, a, alpha))
					return 1;
			}
		}
		for (int j = nf; j < J; j++)
			if (two_pass(j))
				return 1;
		return 0;
	}
	for (int j = J; j > nf; j--)
		if (two_pass(j))
			return 1;
	if (nf > 0) {
		if (fused_scratch(f, d, batch, bs, &C, LL))
			return 1;
		for (int j = nf; j >= 1; j--) {
			EawLevelArgs a;
			a.W = ge.Wo(j - 1);
			a.H = ge.Ho(j - 1);
			a.batch = batch;
			a.ll = j == nf ? C : LL[(nf - j - 1) & 1];
			a.pll = j == nf ? W : pll;
			a.bi_ll = j == nf ? (long)W * H : bll;
			a.det = C;
			a.pd = W;
			a.bi_det = (long)W * H;
			if (j == 1) {
				a.out = (float *)d.p;
				a.pout = d.sx / 4;
				a.bi_out = bs / 4;
			} else {
				a.out = LL[(nf - j) & 1];
				a.pout = pll;
				a.bi_out = bll;
			}
			a.wH = wb + f.offH[j - 1];
			a.wV = wb + f.offV[j - 1];
			a.bi_w = ws;
			if (level_launch(f.wavelet, true, a, alpha))
				return 1;
		}
	}
	return 0;
}

int eaw2d(EawWavelet wv, bool inverse, int layout, void *ptr, int stride_x, int stride_y, const Geom &ge, int *jp, int decompose_one,
	int zero_padding, float *weights, float alpha)
{
	EawFrame f;
	f.wavelet = wv;
	f.layout = layout;
	f.ge = ge;
	f.J = eaw_levels(inverse, ge, decompose_one, jp);
	eaw_layout(&f);
	if (f.J == 0 || ge.sox == 0 || ge.soy == 0)
		return 0;
	const bool dev = dwt_hip_is_device_pointer(ptr);
	if (dev != (bool)dwt_hip_is_device_pointer(weights))
		return fail("the image and the weights must both be host or both be device memory");
	// the frame the transform touches: Mallat the outer frame, interleaved the inner one
	const int fw = layout == DWT_HIP_EAW_MALLAT ? ge.sox : ge.six, fh = layout == DWT_HIP_EAW_MALLAT ? ge.soy : ge.siy;
	if (dev && stride_y == 4 && stride_x % 4 == 0 && (uintptr_t)ptr % 4 == 0 && (fh == 1 || stride_x >= 4l * fw))
		return run_device(inverse, f, Img{(char *)ptr, fh == 1 ? align_up(4l * fw, 4) : (long)stride_x, 4}, 1, 0, weights, f.total,
			zero_padding, alpha);
	// host memory, strided or unaligned device images: the staging detour (dwt_backend.h)
	const Frame fr{ptr, stride_x, stride_y, 4, fw, fh, dev};
	Img A;
	float *wd = weights;
	if (frame_stage(fr, g.frame_a, &A))
		return 1;
	if (!dev) {
		if (grow(g.eaw_w, std::max<size_t>((size_t)f.total * 4, 4)))
			return 1;
		wd = (float *)g.eaw_w.p;
		if (inverse)
			HIP_TRY(hipMemcpyAsync(wd, weights, (size_t)f.total * 4, hipMemcpyHostToDevice, g.stream));
	}
	if (run_device(inverse, f, A, 1, 0, wd, f.total, zero_padding, alpha))
		return 1;
	if (!dev && !inverse)
		HIP_TRY(hipMemcpyAsync(weights, wd, (size_t)f.total * 4, hipMemcpyDeviceToHost, g.stream));
	return frame_unpack(fr, A.p, A.sx);
}

// the argument checks of dwt_hip_eaw53_2d / dwt_hip_eaw97_2d, then the call
int eaw2d_checked(EawWavelet wv, int inverse, int layout, void *ptr, int stride_x, int stride_y, int size_o_x, int size_o_y, int size_i_x,
	int size_i_y, int *j, int decompose_one, int zero_padding, float *weights, float alpha)
{
	if (check_inited())
		return 1;
	if (layout != DWT_HIP_EAW_MALLAT && layout != DWT_HIP_EAW_INTERLEAVED)
		return fail("EAW: unknown layout %d", layout);
	if (!ptr || !j)
		return fail("null pointer argument");
	if (size_o_x < 0 || size_o_y < 0 || size_i_x < 0 || size_i_y < 0 || size_i_x > size_o_x || size_i_y > size_o_y)
		return fail("bad sizes: outer %d x %d, inner %d x %d", size_o_x, size_o_y, size_i_x, size_i_y);
	if (stride_y < 4 || stride_x < 4)
		return fail("bad strides: %d, %d bytes", stride_x, stride_y);
	int jj = *j;
	const Geom ge{size_o_x, size_o_y, size_i_x, size_i_y};
	if (eaw_levels(inverse != 0, ge, decompose_one, &jj) > 0 && !weights && size_o_x > 0 && size_o_y > 0)
		return fail("null weights");
	return eaw2d(wv, inverse != 0, layout, ptr, stride_x, stride_y, ge, j, decompose_one, zero_padding, weights, alpha);
}

// the same of the batch entries
int eaw2d_batch_checked(EawWavelet wv, int inverse, void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y, int *j,
	int decompose_one, float *weights, size_t weights_stride, float alpha)
{
	if (check_inited())
		return 1;
	if (!ptr || !j || batch < 0 || size_x < 0 || size_y < 0)
		return fail("EAW batch: bad arguments");
	if (!dwt_hip_is_device_pointer(ptr) || (batch > 0 && size_x > 0 && size_y > 0 && !dwt_hip_is_device_pointer(weights)))
		return fail("EAW batch: images and weights must be device memory");
	if ((uintptr_t)ptr % 4 || stride_x % 4 || batch_stride % 4 || stride_x < 4l * size_x || (batch > 1 && batch_stride < (size_t)stride_x * size_y) ||
		batch_stride > (size_t)LONG_MAX / 2)
		return fail("EAW batch: images must be dense, aligned and apart (stride %d, batch stride %zu)", stride_x, batch_stride);
	EawFrame f;
	f.wavelet = wv;
	f.layout = DWT_HIP_EAW_MALLAT;
	f.ge = Geom{size_x, size_y, size_x, size_y};
	f.J = eaw_levels(inverse != 0, f.ge, decompose_one, j);
	eaw_layout(&f);
	if (batch > 1 && weights_stride < (size_t)f.total)
		return fail("EAW batch: weights stride %zu floats, one image takes %ld", weights_stride, f.total);
	if (batch == 0 || f.J == 0 || size_x == 0 || size_y == 0)
		return 0;
	return run_device(inverse != 0, f, Img{(char *)ptr, stride_x, 4}, batch, (long)batch_stride, weights, (long)weights_stride, 0, alpha);
}

} // namespace

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

long dwt_hip_eaw53_weights_layout(int layout, int size_o_x, int size_o_y, int size_i_x, int size_i_y, int j, long *off_h, long *off_v)
{
	if ((layout != DWT_HIP_EAW_MALLAT && layout != DWT_HIP_EAW_INTERLEAVED) || j < 0 || j > 32 || size_i_x < 0 || size_i_y < 0 ||
		size_i_x > size_o_x || size_i_y > size_o_y)
		return -1;
	EawFrame f;
	f.wavelet = kEaw53; // the layout does not depend on the wavelet
	f.layout = layout;
	f.ge = Geom{size_o_x, size_o_y, size_i_x, size_i_y};
	f.J = j;
	eaw_layout(&f);
	for (int k = 0; k < j; k++) {
		if (off_h)
			off_h[k] = f.offH[k];
		if (off_v)
			off_v[k] = f.offV[k];
	}
	return f.total;
}

int dwt_hip_eaw53_2d(int inverse, int layout, void *ptr, int stride_x, int stride_y, int size_o_x, int size_o_y, int size_i_x,
	int size_i_y, int *j, int decompose_one, int zero_padding, float *weights, float alpha)
{
	return eaw2d_checked(kEaw53, inverse, layout, ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j, decompose_one,
		zero_padding, weights, alpha);
}

int dwt_hip_eaw53_2d_batch(int inverse, void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y, int *j,
	int decompose_one, float *weights, size_t weights_stride, float alpha)
{
	return eaw2d_batch_checked(kEaw53, inverse, ptr, batch_stride, batch, stride_x, size_x, size_y, j, decompose_one, weights,
		weights_stride, alpha);
}

int dwt_hip_eaw97_2d(int inverse, void *ptr, int stride_x, int stride_y, int size_o_x, int size_o_y, int size_i_x, int size_i_y, int *j,
	int decompose_one, int zero_padding, float *weights, float alpha)
{
	return eaw2d_checked(kEaw97, inverse, DWT_HIP_EAW_MALLAT, ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j,
		decompose_one, zero_padding, weights, alpha);
}

int dwt_hip_eaw97_2d_batch(int inverse, void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y, int *j,
	int decompose_one, float *weights, size_t weights_stride, float alpha)
{
	return eaw2d_batch_checked(kEaw97, inverse, ptr, batch_stride, batch, stride_x, size_x, size_y, j, decompose_one, weights,
		weights_stride, alpha);
}

} // extern "C"
#pragma GCC visibility pop
