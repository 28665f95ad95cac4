// dwt_backend_quant.hip -- deadzone quantization of coefficient planes to integer indices and back, the per-band counters,
// the step tables from the synthesis norms, the code-block layout and its bit-plane map, and their C-ABI
// (include/libdwt_hip.h).
//
// One call is one launch of k_quant or k_codeblock_bitplanes (dwt_quant.hip) on the context's stream.  The slots, the level
// rule and the rectangles are those of the band operators, taken through dwt_hip_band_levels / dwt_hip_band_geometry.
// The step table(s) -- as reciprocals for the quantizer -- cross to the context's workspace in one small copy in front of
// the launch; the band counters live behind them, cleared before the launch, in a few copies that the workgroups spread
// over and the driver folds on the host.  Each side lies in host or in device memory on its own; a host side is mirrored
// like a side of the pixel front end (mirror / mirror_back).
#include "dwt_backend.h"

#include <climits>
#include <cmath>

namespace dwtb {

namespace {

static_assert(QUANT_GRID_ROWS == DWT_HIP_QUANT_GRID_ROWS && QUANT_GRID_BATCH == DWT_HIP_QUANT_GRID_BATCH &&
		CODEBLOCK_GRID * CODEBLOCK_WG_BLOCKS == DWT_HIP_CODEBLOCK_GRID_BLOCKS, "the header states the kernels' constants");
static_assert((int)kCoefS == DWT_HIP_COEF_S && (int)kCoefH == DWT_HIP_COEF_H && (int)kIndexI16 == DWT_HIP_INDEX_I16 && (int)kIndexI32 == DWT_HIP_INDEX_I32,
	"element types");
static_assert(DWT_HIP_QUANT_MAX_LEVELS <= QUANT_MAX_LEVELS && 3 * QUANT_MAX_LEVELS + 1 == BAND_MAX_SLOTS, "slot tables");

// one side's frames: `batch` frames of W x H elements of es bytes
struct Plane {
	const void *p;
	long bs, pitch;
	int es;
	Side side;
};

int plane_check(Plane *pl, const char *what, const void *p, size_t bs, size_t pitch, int es, int batch, int W, int H)
{
	if (!p)
		return fail("null pointer argument");
	const size_t lim = (size_t)1 << 46;
	if (bs > lim || pitch > lim)
		return fail("quant: bad strides of the %s", what);
	// a stride that no element is reached by does not count
	pl->p = p, pl->es = es, pl->bs = batch > 1 ? (long)bs : 0, pl->pitch = H > 1 ? (long)pitch : 0;
	if ((uintptr_t)p % es || pl->bs % es || pl->pitch % es)
		return fail("quant: the %s' address and strides are multiples of the element size (%d bytes)", what, es);
	const long row = (long)W * es;
	long one = row;
	if ((H > 1 && pl->pitch < row) || !mul_add(&one, std::max(H - 1, 0), pl->pitch))
		return fail("quant: bad row pitch of the %s (%zu bytes for %d elements of %d)", what, pitch, W, es);
	if (batch > 1 && pl->bs < one)
		return fail("quant: the %s' frames must be apart (batch stride %zu bytes, a frame takes %ld)", what, bs, one);
	long extent = one;
	if (!mul_add(&extent, std::max(batch - 1, 0), pl->bs))
		return fail("quant: bad strides of the %s", what);
	pl->side = Side{p, (size_t)extent, (H < 2 || pl->pitch == row) && (batch < 2 || pl->bs == one)};
	return 0;
}

// the frames of a call and their slots
struct Frames {
	int batch, W, H, J, ns;
	int xywh[4 * BAND_MAX_SLOTS];
	bool empty() const { return batch == 0 || W == 0 || H == 0; }
};

int frames_check(Frames *f, int batch, int W, int H, int j_max)
{
	if (batch < 0 || W < 0 || H < 0)
		return fail("quant: bad sizes (%d frames of %d x %d)", batch, W, H);
	f->batch = batch, f->W = W, f->H = H;
	f->J = dwt_hip_band_levels(W, H, j_max);
	f->ns = dwt_hip_band_geometry(W, H, W, H, j_max, f->xywh);
	if (f->J < 0 || f->ns != 3 * f->J + 1)
		return fail("quant: bad sizes (%d x %d, j_max %d)", W, H, j_max);
	return 0;
}

int type_sizes(int coef_type, int index_type, int *ces, int *ies)
{
	if (coef_type != DWT_HIP_COEF_S && coef_type != DWT_HIP_COEF_H)
		return fail("quant: unknown coefficient type %d", coef_type);
	if (index_type != DWT_HIP_INDEX_I16 && index_type != DWT_HIP_INDEX_I32)
		return fail("quant: unknown index type %d", index_type);
	*ces = quant_coef_es(coef_type), *ies = quant_index_es(index_type);
	return 0;
}

// a checked quantizer call
struct QuantCall {
	Frames f;
	int coef_type, index_type;
	Plane coef, index;
	bool in_place;
};

int quant_check(QuantCall *c, int coef_type, const void *coef, size_t coef_bs, size_t coef_pitch, int index_type, const void *index,
	size_t index_bs, size_t index_pitch, int batch, int W, int H, int j_max)
{
	int ces, ies;
	if (type_sizes(coef_type, index_type, &ces, &ies) || frames_check(&c->f, batch, W, H, j_max) ||
	    plane_check(&c->coef, "coefficients", coef, coef_bs, coef_pitch, ces, batch, W, H) ||
	    plane_check(&c->index, "indices", index, index_bs, index_pitch, ies, batch, W, H))
		return 1;
	c->coef_type = coef_type, c->index_type = index_type;
	// (binary32 <-> int32 only: binary16 and int16 share a size too, but the header promises no in-place call for them)
	c->in_place = coef == index && coef_type == DWT_HIP_COEF_S && index_type == DWT_HIP_INDEX_I32 && c->coef.pitch == c->index.pitch &&
	              c->coef.bs == c->index.bs;
	if (!c->in_place && !c->f.empty() && overlap(coef, c->coef.side.extent, index, c->index.side.extent))
		return fail("quant: the coefficients and the indices overlap (in place: binary32 and int32 at one address with equal strides)");
	return 0;
}

// which side moves by 16-byte accesses -- from addresses and strides alone
void quant_route(QuantArgs *a)
{
	const bool want = g.quant_wide != 0;
	a->wide_coef = want && all16({(uintptr_t)a->coef, (uintptr_t)a->coef_bs, (uintptr_t)a->coef_pitch});
	a->wide_index = want && all16({(uintptr_t)a->index, (uintptr_t)a->index_bs, (uintptr_t)a->index_pitch});
}

void quant_args(const QuantCall &c, char *coef, char *index, QuantArgs *a)
{
	*a = QuantArgs{};
	a->coef = coef, a->coef_pitch = c.coef.pitch, a->coef_bs = c.coef.bs;
	a->index = index, a->index_pitch = c.index.pitch, a->index_bs = c.index.bs;
	a->batch = c.f.batch, a->W = c.f.W, a->H = c.f.H, a->J = c.f.J;
	a->xb[0] = c.f.W, a->yb[0] = c.f.H;
	for (int j = 1; j <= c.f.J; j++) {
		a->xb[j] = c.f.xywh[4 * (3 * (j - 1) + 0) + 0]; // HL(j) starts the H half of the columns
		a->yb[j] = c.f.xywh[4 * (3 * (j - 1) + 1) + 1]; // LH(j) that of the rows
	}
	quant_route(a);
}

int steps_check(const Frames &f, const float *steps, size_t table_stride, int *n_tables)
{
	if (!steps)
		return fail("quant: null step table");
	if (table_stride > (size_t)INT_MAX || (table_stride && table_stride < (size_t)f.ns))
		return fail("quant: table stride %zu, one table takes %d steps", table_stride, f.ns);
	*n_tables = table_stride && f.batch > 0 ? f.batch : 1;
	for (int t = 0; t < *n_tables; t++)
		for (int k = 0; k < f.ns; k++) {
			const float s = steps[(size_t)t * table_stride + k];
			if (!(s > 0.f) || !std::isfinite(s))
				return fail("quant: step %g in slot %d of table %d (a step is finite and > 0)", (double)s, k, t);
		}
	return 0;
}

int stat_copies_for(const Frames &f)
{
	int copies = 16;
	while (copies > 1 && (size_t)copies * f.batch * f.ns * QUANT_STAT_WORDS * 8 > ((size_t)4 << 20))
		copies >>= 1;
	return copies;
}

int quant_run_call(const QuantCall &c, bool inverse, const float *steps, size_t table_stride, int n_tables, float r, long long *stats)
{
	const Frames &f = c.f;
	const size_t n_stat = (size_t)f.batch * f.ns * QUANT_STAT_WORDS;
	if (stats)
		std::fill(stats, stats + n_stat, 0ll);
	if (f.empty())
		return 0;
	if (check_inited())
		return 1;
	// the workspace: the tables, then the counters' copies
	const size_t n_tab = (size_t)n_tables * f.ns, tab_bytes = (size_t)align_up((long)n_tab * 4, 256);
	const int copies = stats ? stat_copies_for(f) : 0;
	if (grow(g.q_ws, tab_bytes + (size_t)copies * n_stat * 8))
		return 1;
	const Plane &src = inverse ? c.index : c.coef, &dst = inverse ? c.coef : c.index;
	Buf &src_buf = inverse ? g.q_index : g.q_coef, &dst_buf = inverse ? g.q_coef : g.q_index;
	char *sp, *dp;
	bool src_host, dst_host;
	if (mirror(src.side, src_buf, true, &sp, &src_host))
		return 1;
	if (c.in_place)
		dp = sp, dst_host = src_host;
	else if (mirror(dst.side, dst_buf, !dst.side.dense, &dp, &dst_host))
		return 1;
	// (pageable memory: the copy has read it when it returns)
	static thread_local std::vector<float> packed;
	packed.resize(n_tab);
	for (int t = 0; t < n_tables; t++)
		for (int k = 0; k < f.ns; k++) {
			const float s = steps[(size_t)t * table_stride + k];
			packed[(size_t)t * f.ns + k] = inverse ? s : 1.0f / s;
		}
	HIP_TRY(hipMemcpyAsync(g.q_ws.p, packed.data(), n_tab * 4, hipMemcpyHostToDevice, g.stream));
	QuantArgs a;
	quant_args(c, inverse ? dp : sp, inverse ? sp : dp, &a);
	a.tab = (const float *)g.q_ws.p;
	a.tstride = n_tables > 1 ? f.ns : 0;
	a.r = r;
	a.nt_out = nt_for(dst.side.extent);
	if (stats) {
		a.stats = (unsigned long long *)((char *)g.q_ws.p + tab_bytes);
		a.stat_copies = copies;
		HIP_TRY(hipMemsetAsync(a.stats, 0, (size_t)copies * n_stat * 8, g.stream));
	}
	if (launched(launch_quant(c.coef_type, c.index_type, inverse, a, g.stream), "quant", inverse ? "dequantize" : "quantize"))
		return 1;
	if (dst_host && mirror_back(dst.side, c.in_place ? src_buf : dst_buf))
		return 1;
	if (stats) {
		static thread_local std::vector<unsigned long long> raw;
		raw.resize((size_t)copies * n_stat);
		HIP_TRY(hipMemcpyAsync(raw.data(), a.stats, raw.size() * 8, hipMemcpyDeviceToHost, g.stream));
		HIP_TRY(hipStreamSynchronize(g.stream));
		for (int cp = 0; cp < copies; cp++)
			for (size_t i = 0; i < n_stat; i++) {
				const long long v = (long long)raw[(size_t)cp * n_stat + i];
				stats[i] = i % QUANT_STAT_WORDS == 1 ? std::max(stats[i], v) : stats[i] + v;
			}
	} else if (src_host || dst_host) {
		HIP_TRY(hipStreamSynchronize(g.stream));
	}
	return 0;
}

// ---- the synthesis norms (host arithmetic in double)
struct Lifting {
	int K;           // lifting steps of the inverse; step s acts on the samples of parity par[s]
	double ic[4];
	int par[4];
	double even, odd; // the inverse's scaling of the L (even) and the H (odd) coefficients
};

int lifting_of(int wavelet, Lifting *w)
{
	switch (wavelet) {
	case DWT_HIP_CDF97_S: {
		// dwt_lift.h, Cdf97S: -u2, p2, -u1, p1; even *= 1 / zeta (a float division), odd *= zeta
		const float zeta = 1.1496043988602f;
		*w = Lifting{4, {-0.4435068520439f, -0.8829110755309f, 0.0529801185729f, 1.58613434342059f}, {0, 1, 0, 1}, 1.0f / zeta, zeta};
		return 0;
	}
	case DWT_HIP_CDF53_S:
		*w = Lifting{2, {-0.25f, 0.5f, 0, 0}, {0, 1, 0, 0}, 0.70710678118654752440f, 1.41421356237309504880f};
		return 0;
	case DWT_HIP_INTERP53_S:
		*w = Lifting{1, {0.5f, 0, 0, 0}, {1, 0, 0, 0}, 0.70710678118654752440f, 1.41421356237309504880f};
		return 0;
	}
	return fail("quant: wavelet %d has no float synthesis norms (DWT_HIP_CDF97_S, _CDF53_S, _INTERP53_S)", wavelet);
}

// one inverse level of a line of n = 2h samples: l[0 .. h), hi[0 .. h) -> x[0 .. n), whole-sample reflection at the ends
void inverse_level(const Lifting &w, const std::vector<double> &l, const std::vector<double> &hi, std::vector<double> *x)
{
	const int h = (int)l.size(), n = 2 * h;
	x->assign(n, 0.0);
	for (int i = 0; i < h; i++)
		(*x)[2 * i] = l[i] * w.even, (*x)[2 * i + 1] = hi[i] * w.odd;
	for (int s = 0; s < w.K; s++)
		for (int i = w.par[s]; i < n; i += 2) {
			const double left = (*x)[i == 0 ? 1 : i - 1], right = (*x)[i == n - 1 ? n - 2 : i + 1];
			(*x)[i] += w.ic[s] * (left + right);
		}
}

double synthesis_norm(const Lifting &w, int j, bool high)
{
	std::vector<double> l(64, 0.0), hi(64, 0.0), x;
	(high ? hi : l)[32] = 1.0;
	for (int level = j; level >= 1; level--) {
		inverse_level(w, l, hi, &x);
		l = x;
		hi.assign(l.size(), 0.0);
	}
	double sum = 0;
	for (double v : l)
		sum += v * v;
	return sqrt(sum);
}

int norms(int wavelet, int levels, double *norm_l, double *norm_h)
{
	Lifting w;
	if (levels < 0 || levels > DWT_HIP_QUANT_MAX_LEVELS)
		return fail("quant: %d levels (0 .. %d)", levels, DWT_HIP_QUANT_MAX_LEVELS);
	if (lifting_of(wavelet, &w))
		return 1;
	for (int j = 1; j <= levels; j++) {
		norm_l[j - 1] = synthesis_norm(w, j, false);
		norm_h[j - 1] = synthesis_norm(w, j, true);
	}
	return 0;
}

// ---- code-blocks
int layout(const Frames &f, int cbx, int cby, int *first, int *blocks_x)
{
	if (cbx < 2 || cbx > 10 || cby < 2 || cby > 10 || cbx + cby > 12)
		return fail("code-blocks of 2^%d x 2^%d samples (each exponent 2 .. 10, their sum at most 12)", cbx, cby);
	long total = 0;
	for (int k = 0; k < f.ns; k++) {
		const int w = f.xywh[4 * k + 2], h = f.xywh[4 * k + 3];
		const long nx = w > 0 && h > 0 ? (w + (1l << cbx) - 1) >> cbx : 0, ny = nx ? (h + (1l << cby) - 1) >> cby : 0;
		if (first)
			first[k] = (int)total;
		if (blocks_x)
			blocks_x[k] = (int)nx;
		total += nx * ny;
		if (total > INT_MAX)
			return fail("frame too large (%ld code-blocks)", total);
	}
	if (first)
		first[f.ns] = (int)total;
	return 0;
}

} // namespace

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_quant_norms(int wavelet, int levels, double *norm_l, double *norm_h)
{
	if (!norm_l || !norm_h)
		return fail("null pointer argument");
	return norms(wavelet, levels, norm_l, norm_h);
}

int dwt_hip_quant_steps(int wavelet, int levels, float base_step, float *steps)
{
	if (!steps)
		return fail("null pointer argument");
	if (!(base_step > 0.f) || !std::isfinite(base_step))
		return fail("quant: base step %g (finite and > 0)", (double)base_step);
	double nl[DWT_HIP_QUANT_MAX_LEVELS + 1], nh[DWT_HIP_QUANT_MAX_LEVELS + 1];
	if (norms(wavelet, levels, nl + 1, nh + 1))
		return 1;
	nl[0] = 1.0; // (no level: the samples themselves)
	for (int j = 1; j <= levels; j++) {
		steps[3 * (j - 1) + 0] = (float)((double)base_step / (nh[j] * nl[j]));
		steps[3 * (j - 1) + 1] = (float)((double)base_step / (nl[j] * nh[j]));
		steps[3 * (j - 1) + 2] = (float)((double)base_step / (nh[j] * nh[j]));
	}
	steps[3 * levels] = (float)((double)base_step / (nl[levels] * nl[levels]));
	return 0;
}

int dwt_hip_quantize_batch(int coef_type, const void *coef, size_t coef_batch_stride, size_t coef_row_pitch, int index_type, void *index,
	size_t index_batch_stride, size_t index_row_pitch, int batch, int size_x, int size_y, int j_max, const float *steps,
	size_t table_stride, long long *stats)
{
	QuantCall c;
	int n_tables;
	if (quant_check(&c, coef_type, coef, coef_batch_stride, coef_row_pitch, index_type, index, index_batch_stride, index_row_pitch, batch,
			size_x, size_y, j_max) ||
	    steps_check(c.f, steps, table_stride, &n_tables))
		return 1;
	if (stats && dwt_hip_is_device_pointer(stats))
		return fail("quant: the band counters go to host memory");
	return quant_run_call(c, false, steps, table_stride, n_tables, 0.f, stats);
}

int dwt_hip_dequantize_batch(int index_type, const void *index, size_t index_batch_stride, size_t index_row_pitch, int coef_type, void *coef,
	size_t coef_batch_stride, size_t coef_row_pitch, int batch, int size_x, int size_y, int j_max, const float *steps,
	size_t table_stride, float r)
{
	QuantCall c;
	int n_tables;
	if (quant_check(&c, coef_type, coef, coef_batch_stride, coef_row_pitch, index_type, index, index_batch_stride, index_row_pitch, batch,
			size_x, size_y, j_max) ||
	    steps_check(c.f, steps, table_stride, &n_tables))
		return 1;
	if (!(r >= 0.f && r < 1.f))
		return fail("quant: reconstruction offset %g (0 <= r < 1)", (double)r);
	return quant_run_call(c, true, steps, table_stride, n_tables, r, nullptr);
}

int dwt_hip_quant_route(int coef_type, const void *coef, size_t coef_batch_stride, size_t coef_row_pitch, int index_type, const void *index,
	size_t index_batch_stride, size_t index_row_pitch, int batch, int size_x, int size_y)
{
	QuantCall c;
	if (quant_check(&c, coef_type, coef, coef_batch_stride, coef_row_pitch, index_type, index, index_batch_stride, index_row_pitch, batch,
			size_x, size_y, 0))
		return -1;
	QuantArgs a;
	quant_args(c, (char *)coef, (char *)index, &a);
	return (a.wide_coef ? DWT_HIP_QUANT_WIDE_COEF : 0) | (a.wide_index ? DWT_HIP_QUANT_WIDE_INDEX : 0);
}

int dwt_hip_codeblock_layout(int size_x, int size_y, int j_max, int cb_log2_x, int cb_log2_y, int *first, int *blocks_x)
{
	Frames f;
	int total[BAND_MAX_SLOTS + 1];
	if (frames_check(&f, 1, size_x, size_y, j_max) || layout(f, cb_log2_x, cb_log2_y, total, blocks_x))
		return -1;
	if (first)
		std::copy(total, total + f.ns + 1, first);
	return total[f.ns];
}

int dwt_hip_codeblock_bitplanes_batch(int index_type, const void *index, size_t index_batch_stride, size_t index_row_pitch, int batch,
	int size_x, int size_y, int j_max, int cb_log2_x, int cb_log2_y, unsigned char *planes, size_t planes_frame_stride)
{
	int ces, ies;
	Frames f;
	Plane idx;
	CodeblockArgs a{};
	if (type_sizes(DWT_HIP_COEF_S, index_type, &ces, &ies) || frames_check(&f, batch, size_x, size_y, j_max) ||
	    plane_check(&idx, "indices", index, index_batch_stride, index_row_pitch, ies, batch, size_x, size_y) ||
	    layout(f, cb_log2_x, cb_log2_y, a.first, a.blocks_x))
		return 1;
	if (!planes)
		return fail("null pointer argument");
	const long total = a.first[f.ns];
	if (planes_frame_stride > ((size_t)1 << 46) || (batch > 1 && planes_frame_stride < (size_t)total))
		return fail("code-blocks: frame stride %zu of the map, a frame has %ld blocks", planes_frame_stride, total);
	if (f.empty() || total == 0)
		return 0;
	const size_t map_extent = (size_t)(batch - 1) * planes_frame_stride + total;
	if (overlap(index, idx.side.extent, planes, map_extent))
		return fail("code-blocks: the indices and the map overlap");
	if (check_inited())
		return 1;
	char *ip;
	bool idx_host;
	if (mirror(idx.side, g.q_index, true, &ip, &idx_host))
		return 1;
	// a host map: a dense one on the device, whose rows go back to the frames' places (the bytes between them are left alone)
	const bool map_host = !dwt_hip_is_device_pointer(planes);
	if (map_host && grow(g.q_planes, (size_t)batch * total))
		return 1;
	a.index = ip, a.index_pitch = idx.pitch, a.index_bs = idx.bs;
	a.batch = batch, a.nslots = f.ns, a.cbx = cb_log2_x, a.cby = cb_log2_y;
	a.wide = g.quant_wide != 0 && all16({(uintptr_t)a.index, (uintptr_t)a.index_bs, (uintptr_t)a.index_pitch});
	for (int k = 0; k < f.ns; k++)
		a.x0[k] = f.xywh[4 * k], a.y0[k] = f.xywh[4 * k + 1], a.w[k] = f.xywh[4 * k + 2], a.h[k] = f.xywh[4 * k + 3];
	a.planes = map_host ? (unsigned char *)g.q_planes.p : planes;
	a.planes_bs = map_host ? total : (batch > 1 ? (long)planes_frame_stride : 0);
	if (launched(launch_codeblock_bitplanes(index_type, a, g.stream), "code-block", "bit-planes"))
		return 1;
	if (map_host)
		HIP_TRY(hipMemcpy2DAsync(planes, batch > 1 ? planes_frame_stride : (size_t)total, g.q_planes.p, (size_t)total, (size_t)total, (size_t)batch,
			hipMemcpyDeviceToHost, g.stream));
	if (map_host || idx_host)
		HIP_TRY(hipStreamSynchronize(g.stream));
	return 0;
}

} // extern "C"
#pragma GCC visibility pop
