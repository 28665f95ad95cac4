// dwt_backend_features.hip -- the per-subband feature vectors (dwt_util_wps_s, _maxidx_s, _mean_s, _med_s, _var_s,
// _stdev_s, _skew_s, _kurt_s, _maxnorm_s, _lpnorm_s, _norm_s and their dwt_util_band_*_s primitives,
// src/libdwt.c:23086-23786) on the device, and their C-ABI (include/libdwt_hip.h).
//
// The bands are those of dwt_util_subband (src/libdwt.c:20731): levels 1 .. j_max-1 -- level j_max itself is NOT visited,
// as in the reference -- HL, LH, HH within a level, empty bands skipped.  The kernels (dwt_features.hip) reduce where
// the coefficients lie and leave raw sums in double; the few bytes per band cross to the host, which finishes them in
// float exactly as the reference writes it (finish_band): equal sums give equal features.  Dense rows of up to N1D_MAX
// samples take ONE launch; images and longer rows a fixed set of launches, whatever the batch: pass 1 and its fold,
// pass 2 and its fold when a central moment is asked for, four histogram / pick pairs when the median is.  Host memory
// and strided device images are packed into a dense device image first (frame_pack, dwt_backend.h).
#include "dwt_backend.h"

#include <climits>
#include <cmath>

namespace dwtb {

namespace {

typedef unsigned long long u64;

constexpr unsigned kAllFeatures = (1u << DWT_HIP_FEATURE_COUNT) - 1;
constexpr unsigned kMomentFeatures = DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_VAR) | DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_STDEV) |
	DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_SKEW) | DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_KURT);

struct Band {
	int x0, y0, w, h, j;
};

// the non-empty detail bands of levels 1 .. j_max-1 in the reference's order (bands == nullptr: count only)
int enum_bands(const Geom &ge, int j_max, Band *bands)
{
	int n = 0;
	for (int j = 1; j < j_max && j < 31; j++) { // (beyond 31 halvings every H side is 0)
		const int hx = ge.Wi(j - 1) / 2, hy = ge.Hi(j - 1) / 2, lx = ge.Wi(j), ly = ge.Hi(j), ox = ge.Wo(j), oy = ge.Ho(j);
		const Band three[3] = {{ox, 0, hx, ly, j}, {0, oy, lx, hy, j}, {ox, oy, hx, hy, j}};
		for (const Band &b : three)
			if (b.w && b.h) {
				if (bands)
					bands[n] = b;
				n++;
			}
	}
	return n;
}

// a moment about a given centre / with another exponent (dwt_util_band_moment_s); plain calls: {false, 0, 2}
struct Moment {
	bool use_c = false;
	float c = 0;
	int n = 2;
	bool raw = false; // the moment itself, sum / size, instead of a finished feature
};

// the raw records of this thread's last call (the planes its mask needed), kept for dwt_hip_features_raw_sums
thread_local std::vector<u64> t_host;
thread_local long t_nrec = 0;
thread_local bool t_have[kFeatPlanes] = {};

int popcount(unsigned m) { return __builtin_popcount(m); }

// Everything after the sums, in float, as the reference writes it (src/libdwt.c:23086-23560).  The exponents arrive as
// run-time values through a call that is never inlined, so that powf is libm's and not a folded product.
__attribute__((noinline)) float finish_band(int feature, const u64 *rec, long nrec, long r, int size, int j, float p, int n_exp)
{
	auto sum = [&](int plane) { return (float)__builtin_bit_cast(double, rec[plane * nrec + r]); };
	auto maxnorm = [&] { return __builtin_bit_cast(float, (unsigned)(rec[kFeatKey * nrec + r] >> 32)); };
	auto cmoment = [&](int plane) { return sum(plane) / size; };
	switch (feature) {
	case DWT_HIP_FEATURE_WPS: {
		float s = sum(kFeatS2);
		s /= 1 << j;
		return s;
	}
	case DWT_HIP_FEATURE_MAXIDX:
		return (float)(int)(0xffffffffu - (unsigned)(rec[kFeatKey * nrec + r] & 0xffffffffu));
	case DWT_HIP_FEATURE_MEAN: {
		float s = sum(kFeatS1);
		s /= size;
		return s;
	}
	case DWT_HIP_FEATURE_MED:
		return __builtin_bit_cast(float, (unsigned)rec[kFeatMed * nrec + r]);
	case DWT_HIP_FEATURE_VAR:
		return cmoment(kFeatM2);
	case DWT_HIP_FEATURE_STDEV:
		return sqrtf(cmoment(kFeatM2));
	case DWT_HIP_FEATURE_SKEW:
	case DWT_HIP_FEATURE_KURT: {
		const float stdev = sqrtf(cmoment(kFeatM2));
		const float sm = cmoment(feature == DWT_HIP_FEATURE_SKEW ? kFeatM3 : kFeatM4) / powf(stdev, n_exp);
		return feature == DWT_HIP_FEATURE_SKEW ? sm : sm - 3;
	}
	case DWT_HIP_FEATURE_MAXNORM:
		return maxnorm();
	case DWT_HIP_FEATURE_LPNORM:
	case DWT_HIP_FEATURE_NORM:
		if (p == INFINITY)
			return maxnorm();
		return powf(sum(p == 2.f ? kFeatS2 : kFeatSp), 1 / p);
	}
	return 0.f;
}

// Carves the context's feature workspace.  rec: 8 planes; part: 4 planes; hist: 4 passes of 256 bins per record.
struct Ws {
	u64 *rec = nullptr, *part = nullptr;
	FeatBand *bands = nullptr;
	unsigned *hist = nullptr, *sel = nullptr;
	size_t hist_bytes = 0;
};

int carve(long nrec, long npart, int nb, bool select, Ws *w)
{
	const size_t rec_b = (size_t)kFeatPlanes * nrec * 8, part_b = (size_t)4 * npart * 8, tab_b = align_up((long)nb * sizeof(FeatBand), 256);
	const size_t hist_b = select ? (size_t)4 * nrec * 256 * 4 : 0, sel_b = select ? align_up(nrec * 8, 256) : 0;
	if (grow(g.feat_ws, rec_b + part_b + tab_b + hist_b + sel_b + 256))
		return 1;
	char *p = (char *)g.feat_ws.p;
	w->rec = (u64 *)p;
	p += rec_b;
	w->part = (u64 *)p;
	p += part_b;
	w->bands = (FeatBand *)p;
	p += tab_b;
	w->hist = (unsigned *)p;
	p += hist_b;
	w->sel = (unsigned *)p;
	w->hist_bytes = hist_b;
	return 0;
}

// this driver counts the pack launch of a device frame among its own
int pack(const Frame &f, void *dense, long pitch)
{
	g.stat_launches += f.dev;
	return frame_pack(f, dense, pitch);
}

// how the kernels form the term of plane kFeatSp
int pmode_of(unsigned mask, float p)
{
	const bool lp = (mask & DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_LPNORM)) != 0;
	return !lp || p == 2.f || p == INFINITY ? kFeatPNone : p == 1.f ? kFeatPAbs : kFeatPPow;
}

int finish_records(const u64 *rec, long nrec, int batch, const Band *bands, int nb, unsigned mask, int pmode, float p, const Moment &mom,
	float *fv, long fv_stride);

// a band's entry of the device table: cut into slabs, the first of them slab `slab0` of its image
FeatBand cut_slabs(const Band &b, int slab0)
{
	FeatBand t;
	t.x0 = b.x0;
	t.y0 = b.y0;
	t.w = b.w;
	t.h = b.h;
	t.cw = std::min(t.w, FEAT_SLAB_COLS);
	t.rh = std::max(1, FEAT_SLAB / t.cw);
	t.ncc = (t.w + t.cw - 1) / t.cw;
	t.nslab = t.ncc * ((t.h + t.rh - 1) / t.rh);
	t.slab0 = slab0;
	return t;
}

// `batch` dense device images (4-byte elements, pitch d.sx) bstride bytes apart -> fv (HOST memory): per image one
// block of nb floats per feature of `mask` in enum order, images fv_stride floats apart.
int run_device(Img d, long bstride, int batch, const Band *bands, int nb, bool lines, int N, unsigned mask, float p, const Moment &mom,
	float *fv, long fv_stride)
{
	const bool pass2 = (mask & kMomentFeatures) != 0, select = (mask & DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_MED)) != 0;
	const int pmode = pmode_of(mask, p);
	const long nrec = (long)batch * nb;
	Ws ws;
	if (lines) {
		if (carve(nrec, 0, 0, false, &ws))
			return 1;
		FeatLineArgs a{};
		a.src = d.p;
		a.line_stride = bstride;
		a.n_lines = batch;
		a.N = N;
		a.nb = nb;
		for (int k = 0; k < nb; k++) {
			a.off[k] = bands[k].x0;
			a.len[k] = bands[k].w;
			if (a.off[k] < 0 || a.len[k] <= 0 || a.off[k] + a.len[k] > N)
				return fail("feature band %d outside its line", k);
		}
		a.rec = ws.rec;
		a.nrec = nrec;
		a.work = (pass2 ? kFeatPass2 : 0) | (select ? kFeatSelect : 0);
		a.pmode = pmode;
		a.p = p;
		if (launched(launch_feat_lines(a, g.stream), "feature", "line"))
			return 1;
	} else {
		static thread_local FeatBand tab[FEAT_MAX_BANDS]; // (outlives the asynchronous copy below; the call ends synchronised)
		int slabs = 0;
		for (int k = 0; k < nb; k++) {
			tab[k] = cut_slabs(bands[k], slabs);
			slabs += tab[k].nslab;
		}
		const long npart = (long)batch * slabs;
		if (carve(nrec, npart, nb, select, &ws))
			return 1;
		HIP_TRY(hipMemcpyAsync(ws.bands, tab, (size_t)nb * sizeof(FeatBand), hipMemcpyHostToDevice, g.stream));
		FeatImgArgs a{};
		a.img = d.p;
		a.pitch = d.sx;
		a.bstride = bstride;
		a.batch = batch;
		a.nb = nb;
		a.slabs = slabs;
		a.bands = ws.bands;
		a.part = ws.part;
		a.rec = ws.rec;
		a.nrec = nrec;
		a.hist = ws.hist;
		a.sel = ws.sel;
		a.pmode = pmode;
		a.p = p;
		a.use_c = mom.use_c;
		a.mn = mom.n;
		a.c = mom.c;
		a.groups = g.feat_groups;
		if (launched(launch_feat_pass1(a, g.stream), "feature", "pass 1") || launched(launch_feat_fold(a, 0, g.stream), "feature", "fold"))
			return 1;
		if (pass2 && (launched(launch_feat_pass2(a, g.stream), "feature", "pass 2") || launched(launch_feat_fold(a, 1, g.stream), "feature", "fold")))
			return 1;
		if (select) {
			HIP_TRY(hipMemsetAsync(ws.hist, 0, ws.hist_bytes, g.stream));
			for (int pass = 0; pass < 4; pass++)
				if (launched(launch_feat_hist(a, pass, g.stream), "feature", "histogram") || launched(launch_feat_pick(a, pass, g.stream), "feature", "pick"))
					return 1;
		}
	}
	return finish_records(ws.rec, nrec, batch, bands, nb, mask, pmode, p, mom, fv, fv_stride);
}

// The raw records of `batch` x nb bands cross to the host -- only the planes the mask needs -- and are finished into fv.
int finish_records(const u64 *rec, long nrec, int batch, const Band *bands, int nb, unsigned mask, int pmode, float p, const Moment &mom,
	float *fv, long fv_stride)
{
	const bool pass2 = (mask & kMomentFeatures) != 0, select = (mask & DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_MED)) != 0;
	bool need[kFeatPlanes] = {};
	need[kFeatS1] = mask & DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_MEAN);
	need[kFeatS2] = mask & (DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_WPS) | DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_NORM) | DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_LPNORM));
	need[kFeatSp] = pmode != kFeatPNone;
	need[kFeatM2] = pass2;
	need[kFeatM3] = mask & DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_SKEW);
	need[kFeatM4] = mask & DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_KURT);
	need[kFeatKey] = mask & (DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_MAXIDX) | DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_MAXNORM) |
		DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_LPNORM));
	need[kFeatMed] = select;
	std::vector<u64> &host = t_host;
	host.resize((size_t)kFeatPlanes * nrec);
	t_nrec = nrec;
	for (int f = 0; f < kFeatPlanes; f++)
		t_have[f] = need[f];
	for (int f = 0; f < kFeatPlanes; f++)
		if (need[f])
			HIP_TRY(hipMemcpyAsync(host.data() + (size_t)f * nrec, rec + (size_t)f * nrec, (size_t)nrec * 8, hipMemcpyDeviceToHost, g.stream));
	HIP_TRY(hipStreamSynchronize(g.stream));
	for (int b = 0; b < batch; b++) {
		float *out = fv + (long)b * fv_stride;
		for (int f = 0; f < DWT_HIP_FEATURE_COUNT; f++) {
			if (!(mask & (1u << f)))
				continue;
			const float pf = f == DWT_HIP_FEATURE_NORM ? 2.f : p;
			const int n_exp = f == DWT_HIP_FEATURE_SKEW ? 3 : 4;
			for (int k = 0; k < nb; k++)
				out[k] = mom.raw ? (float)__builtin_bit_cast(double, host[(size_t)(f == DWT_HIP_FEATURE_SKEW ? kFeatM3 : f == DWT_HIP_FEATURE_KURT ? kFeatM4 : kFeatM2) * nrec + (long)b * nb + k]) / (bands[k].w * bands[k].h)
				                 : finish_band(f, host.data(), nrec, (long)b * nb + k, bands[k].w * bands[k].h, bands[k].j, pf, n_exp);
			out += nb;
		}
	}
	return 0;
}

int check_request(unsigned mask, const void *ptr, const float *fv, float p)
{
	if (!ptr || !fv)
		return fail("null pointer argument");
	if (!mask || (mask & ~kAllFeatures))
		return fail("bad feature mask 0x%x", mask);
	if ((mask & DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_LPNORM)) && !(p > 0.f))
		return fail("lpnorm takes p > 0 (got %g)", (double)p);
	return 0;
}

// `batch` frames of `fw` x `fh` elements: image b at ptr + b*bstride, rows stride_x bytes apart, elements stride_y.
// Device images that are dense run where they lie; everything else is packed into the context's dense device image.
int stage(const void *ptr, bool dev, long bstride, int batch, long stride_x, long stride_y, int fw, int fh, Img *d, long *dbs)
{
	if (dev && stride_y == 4 && (fh == 1 || stride_x >= 4l * fw) && (batch == 1 || bstride >= (fh == 1 ? 4l * fw : stride_x * (long)fh))) {
		*d = Img{(char *)ptr, fh == 1 ? 4l * fw : stride_x, 4};
		*dbs = bstride;
		return 0;
	}
	const long pitch = frame_pitch(4, fw);
	if (grow(g.frame_a, (size_t)pitch * fh * batch))
		return 1;
	// the whole batch as ONE image of fh * batch rows where its rows are evenly apart: rows of one-row frames, or
	// images that follow each other without a gap
	const bool one = batch == 1 || (fh == 1 ? true : bstride == stride_x * (long)fh);
	const long row_stride = fh == 1 && batch > 1 ? bstride : stride_x;
	const long rows = one ? (long)fh * batch : fh;
	if (dev && rows > INT_MAX)
		return fail("too many rows to pack (%ld)", rows);
	for (int b = 0; b < (one ? 1 : batch); b++)
		if (pack(Frame{(char *)ptr + (long)b * bstride, row_stride, stride_y, 4, fw, (int)rows, dev}, (char *)g.frame_a.p + (long)b * pitch * fh, pitch))
			return 1;
	*d = Img{(char *)g.frame_a.p, pitch, 4};
	*dbs = pitch * fh;
	return 0;
}

// The tail of a call whose feature vector is device memory: `fill` writes `n` blocks of `block` floats, back to back, into
// host memory; they go to fv, `stride` floats apart.  Ends synchronised: the one host vector of the thread is reused by
// the next call.
thread_local std::vector<float> t_host_fv;
template <class F>
int to_device_fv(float *fv, long stride, long block, int n, F fill)
{
	std::vector<float> &host_fv = t_host_fv;
	host_fv.resize((size_t)block * n);
	if (fill(host_fv.data()))
		return 1;
	HIP_TRY(hipMemcpy2DAsync(fv, (size_t)(n > 1 ? stride : block) * 4, host_fv.data(), (size_t)block * 4, (size_t)block * 4, n, hipMemcpyHostToDevice, g.stream));
	HIP_TRY(hipStreamSynchronize(g.stream));
	return 0;
}

// the common tail: fv in the memory space of the image
int features(unsigned mask, const void *ptr, long bstride, int batch, long stride_x, long stride_y, const Geom &ge, const Band *bands, int nb,
	float p, const Moment &mom, float *fv, long fv_stride, bool fv_follows_ptr)
{
	const bool dev = dwt_hip_is_device_pointer(ptr);
	const bool fv_dev = dwt_hip_is_device_pointer(fv);
	if (fv_follows_ptr ? dev != fv_dev : fv_dev)
		return fail(fv_follows_ptr ? "the image and the feature vector must both be host or both be device memory" : "the feature vector must be host memory");
	if (dev && check_dev_align({ptr}, {stride_x, stride_y, bstride}))
		return 1;
	if (stride_y < 4 || (ge.soy > 1 && stride_x < 4))
		return fail("bad strides: %ld, %ld bytes", stride_x, stride_y);
	if (nb == 0 || batch == 0)
		return 0;
	if (nb > FEAT_MAX_BANDS)
		return fail("too many bands (%d)", nb);
	const int nf = popcount(mask);
	if (batch > 1 && fv_stride < (long)nf * nb)
		return fail("feature stride %ld floats, one image takes %d", fv_stride, nf * nb);
	Img d{nullptr, 0, 4};
	long dbs = 0;
	if (stage(ptr, dev, bstride, batch, stride_x, stride_y, ge.sox, ge.soy, &d, &dbs))
		return 1;
	const bool lines = ge.soy == 1 && ge.sox <= N1D_MAX && nb <= 32 && !mom.raw;
	if (!fv_dev)
		return run_device(d, dbs, batch, bands, nb, lines, ge.sox, mask, p, mom, fv, fv_stride);
	const long block = (long)nf * nb;
	return to_device_fv(fv, fv_stride, block, batch,
		[&](float *host) { return run_device(d, dbs, batch, bands, nb, lines, ge.sox, mask, p, mom, host, block); });
}

bool bad_sizes(int sox, int soy, int six, int siy) { return sox < 0 || soy < 0 || six < 0 || siy < 0 || six > sox || siy > soy; }

// the two entries that take one image with its frame sizes: the bands of dwt_util_subband, every feature of the mask
int features2d(unsigned mask, const void *ptr, int stride_x, int stride_y, int sox, int soy, int six, int siy, int j_max, float p, float *fv,
	bool fv_follows_ptr)
{
	if (check_inited() || check_request(mask, ptr, fv, p))
		return 1;
	if (bad_sizes(sox, soy, six, siy))
		return fail("bad sizes: outer %d x %d, inner %d x %d", sox, soy, six, siy);
	const Geom ge{sox, soy, six, siy};
	Band bands[FEAT_MAX_BANDS];
	const int nb = enum_bands(ge, j_max, bands);
	return features(mask, ptr, 0, 1, stride_x, stride_y, ge, bands, nb, p, Moment{}, fv, 0, fv_follows_ptr);
}

// The features of every level's H (band 0) or L (band 1) plane of the stationary transform of `n_lines` dense device
// lines -> fv (HOST memory), feature k of level l of line y at fv[y*fv_stride + k*levels + l].  Lines the fused kernel
// takes: ONE launch, no coefficient stored.  Otherwise the planes go level by level to library scratch and each level's
// planes through run_device -- what dwt_hip_band_feature does with a stored plane.
int swt_features_device(Wavelet w, unsigned mask, const char *src, long ls, int n_lines, int N, int levels, int band, float p, float *fv,
	long fv_stride)
{
	const int nf = popcount(mask);
	Band bands[SWT_MAX_LEVELS];
	for (int l = 0; l < levels; l++)
		bands[l] = Band{0, 0, N, 1, l}; // (wps divides by 1 << l, as the study calls it)
	if (swt_fused_ok(src, ls, 4, N)) {
		const long nrec = (long)n_lines * levels;
		Ws ws;
		if (carve(nrec, 0, 0, false, &ws))
			return 1;
		SwtLineArgs a{};
		a.src = src;
		a.line_stride = ls;
		a.n_lines = n_lines;
		a.N = N;
		a.levels = levels;
		a.vec = ls % 16 == 0 && (uintptr_t)src % 16 == 0;
		a.rec = ws.rec;
		a.nrec = nrec;
		a.band = band;
		a.work = ((mask & kMomentFeatures) ? kFeatPass2 : 0) | ((mask & DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_MED)) ? kFeatSelect : 0);
		a.pmode = pmode_of(mask, p);
		a.p = p;
		if (launched(launch_swt_lines(w, true, a, g.stream), "feature", "SWT line"))
			return 1;
		return finish_records(ws.rec, nrec, n_lines, bands, levels, mask, a.pmode, p, Moment{}, fv, fv_stride);
	}
	const long pitch = 4l * N, plane = pitch * n_lines;
	if (grow(g.frame_b, (size_t)plane * levels))
		return 1;
	char *planes = (char *)g.frame_b.p;
	if (band ? swt_device(w, src, ls, 4, n_lines, N, 0, levels, nullptr, 4, planes, 4, 2, plane, pitch) // (no H: level passes only)
	         : swt_device(w, src, ls, 4, n_lines, N, 0, levels, planes, 4, nullptr, 4, 0, plane, pitch))
		return 1;
	static thread_local std::vector<float> level_fv;
	level_fv.resize((size_t)nf * n_lines);
	for (int l = 0; l < levels; l++) {
		if (run_device(Img{planes + (size_t)plane * l, pitch, 4}, pitch, n_lines, bands + l, 1, N <= N1D_MAX, N, mask, p, Moment{},
				level_fv.data(), nf))
			return 1;
		for (int y = 0; y < n_lines; y++)
			for (int k = 0; k < nf; k++)
				fv[(long)y * fv_stride + (long)k * levels + l] = level_fv[(size_t)y * nf + k];
	}
	return 0;
}

} // namespace

// The median of |x| over the band (x0, y0, w, h) of each of `batch` dense frames of fw x fh floats -> med (HOST memory):
// the element of rank w*h/2 of the magnitudes, as dwt_util_abs_s + dwt_util_band_med_s give it on a copy.  The images are
// only read: the four rounds of the select run with a key that ignores the sign bit.
int band_abs_median(const void *ptr, long bstride, int batch, long stride_x, int fw, int fh, int x0, int y0, int w, int h, float *med)
{
	const bool dev = dwt_hip_is_device_pointer(ptr);
	if (dev && check_dev_align({ptr}, {stride_x, bstride}))
		return 1;
	Img d{nullptr, 0, 4};
	long dbs = 0;
	if (stage(ptr, dev, bstride, batch, stride_x, 4, fw, fh, &d, &dbs))
		return 1;
	static thread_local FeatBand tab; // (outlives the asynchronous copy below; the call ends synchronised)
	tab = cut_slabs(Band{x0, y0, w, h, 1}, 0);
	Ws ws;
	if (carve(batch, 0, 1, true, &ws))
		return 1;
	HIP_TRY(hipMemcpyAsync(ws.bands, &tab, sizeof(FeatBand), hipMemcpyHostToDevice, g.stream));
	FeatImgArgs a{};
	a.img = d.p;
	a.pitch = d.sx;
	a.bstride = dbs;
	a.batch = batch;
	a.nb = 1;
	a.slabs = tab.nslab;
	a.bands = ws.bands;
	a.rec = ws.rec;
	a.nrec = batch;
	a.hist = ws.hist;
	a.sel = ws.sel;
	a.groups = g.feat_groups;
	a.abs_key = 1;
	HIP_TRY(hipMemsetAsync(ws.hist, 0, ws.hist_bytes, g.stream));
	for (int pass = 0; pass < 4; pass++)
		if (launched(launch_feat_hist(a, pass, g.stream), "feature", "histogram") || launched(launch_feat_pick(a, pass, g.stream), "feature", "pick"))
			return 1;
	std::vector<u64> &host = t_host;
	host.resize((size_t)batch);
	t_nrec = 0; // (no raw sums behind this call)
	HIP_TRY(hipMemcpyAsync(host.data(), ws.rec + (size_t)kFeatMed * batch, (size_t)batch * 8, hipMemcpyDeviceToHost, g.stream));
	HIP_TRY(hipStreamSynchronize(g.stream));
	for (int b = 0; b < batch; b++)
		med[b] = __builtin_bit_cast(float, (unsigned)host[b]);
	return 0;
}

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_count_subbands(int size_o_x, int size_o_y, int size_i_x, int size_i_y, int j_max)
{
	if (bad_sizes(size_o_x, size_o_y, size_i_x, size_i_y))
		return -1;
	return enum_bands(Geom{size_o_x, size_o_y, size_i_x, size_i_y}, j_max, nullptr);
}

int dwt_hip_features2d(unsigned feature_mask, const void *ptr, int stride_x, int stride_y, int size_o_x, int size_o_y, int size_i_x,
	int size_i_y, int j_max, float p, float *fv)
{
	return features2d(feature_mask, ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, p, fv, true);
}

int dwt_hip_features2d_hostfv(unsigned feature_mask, const void *ptr, int stride_x, int stride_y, int size_o_x, int size_o_y, int size_i_x,
	int size_i_y, int j_max, float p, float *fv)
{
	return features2d(feature_mask, ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, p, fv, false);
}

long dwt_hip_features_raw_sums(int plane, double *out, long n)
{
	if (plane < 0 || plane > kFeatM4 || !out || n < 0 || !t_have[plane])
		return -1;
	const long m = std::min(n, t_nrec);
	memcpy(out, t_host.data() + (size_t)plane * t_nrec, (size_t)m * 8);
	return m;
}

int dwt_hip_features2d_batch(unsigned feature_mask, const void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y,
	int j_max, float p, float *fv, size_t fv_stride)
{
	if (check_inited() || check_request(feature_mask, ptr, fv, p))
		return 1;
	if (batch < 0 || size_x < 0 || size_y < 0 || batch_stride > (size_t)LONG_MAX / 2 || fv_stride > (size_t)LONG_MAX / 8)
		return fail("feature batch: bad arguments");
	if (stride_x < 4l * size_x || (batch > 1 && batch_stride < (size_t)stride_x * size_y))
		return fail("feature batch: images must be dense and apart (stride %d, batch stride %zu)", stride_x, batch_stride);
	const Geom ge{size_x, size_y, size_x, size_y};
	Band bands[FEAT_MAX_BANDS];
	const int nb = enum_bands(ge, j_max, bands);
	return features(feature_mask, ptr, (long)batch_stride, batch, stride_x, 4, ge, bands, nb, p, Moment{}, fv, (long)fv_stride, true);
}

int dwt_hip_features1d_batch(unsigned feature_mask, const void *ptr, size_t line_stride, size_t elem_stride, int n_lines, int size,
	int j_max, float p, float *fv, size_t fv_stride)
{
	if (check_inited() || check_request(feature_mask, ptr, fv, p))
		return 1;
	if (n_lines < 0 || size < 0 || line_stride > (size_t)LONG_MAX / 2 || elem_stride > INT_MAX || fv_stride > (size_t)LONG_MAX / 8)
		return fail("feature lines: bad arguments");
	if (elem_stride < 4 || (n_lines > 1 && line_stride < elem_stride * (size_t)size))
		return fail("feature lines: lines must be apart (line stride %zu, element stride %zu)", line_stride, elem_stride);
	const Geom ge{size, 1, size, 1};
	Band bands[FEAT_MAX_BANDS];
	const int nb = enum_bands(ge, j_max, bands);
	// n_lines frames of one row each; strided elements: stage() packs the lines as the rows of one dense image
	return features(feature_mask, ptr, (long)line_stride, n_lines, (long)elem_stride * size, (long)elem_stride, ge, bands, nb, p, Moment{}, fv,
		(long)fv_stride, true);
}

int dwt_hip_swt_features1d_batch(int wavelet, unsigned feature_mask, const void *src, size_t line_stride, size_t elem_stride, int n_lines, int N,
	int levels, int band, float p, float *fv, int fv_line_stride)
{
	Wavelet w;
	if (!wavelet_of(wavelet, &w) || (w != kCdf97S && w != kCdf53S))
		return fail("the SWT takes DWT_HIP_CDF97_S or DWT_HIP_CDF53_S (got wavelet %d)", wavelet);
	if (n_lines < 0 || N < 0 || levels < 0 || levels > SWT_MAX_LEVELS || band < 0 || band > 1 || line_stride > (size_t)LONG_MAX / 2 ||
		elem_stride > INT_MAX || fv_line_stride < 0)
		return fail("SWT features: bad arguments (%d lines of %d samples, %d levels of at most %d, band %d)", n_lines, N, levels,
			SWT_MAX_LEVELS, band);
	if (check_request(feature_mask, src, fv, p))
		return 1;
	if (elem_stride < 4 || (n_lines > 1 && line_stride < elem_stride * (size_t)N))
		return fail("SWT features: lines must be apart (line stride %zu, element stride %zu)", line_stride, elem_stride);
	const int nf = popcount(feature_mask);
	if (n_lines > 1 && fv_line_stride < nf * levels)
		return fail("feature stride %d floats, one line takes %d", fv_line_stride, nf * levels);
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(src);
	if (dev != (bool)dwt_hip_is_device_pointer(fv))
		return fail("the lines and the feature vector must both be host or both be device memory");
	if (dev && check_dev_align({src}, {(long)elem_stride, (long)line_stride}))
		return 1;
	if (n_lines == 0 || N == 0 || levels == 0)
		return 0;
	// dense device lines run where they lie; everything else is packed into the context's dense device image
	Img A;
	long ls = 0;
	if (stage(src, dev, (long)line_stride, n_lines, (long)elem_stride * N, (long)elem_stride, N, 1, &A, &ls))
		return 1;
	const char *d = A.p;
	if (!dev)
		return swt_features_device(w, feature_mask, d, ls, n_lines, N, levels, band, p, fv, fv_line_stride);
	const long block = (long)nf * levels;
	return to_device_fv(fv, fv_line_stride, block, n_lines,
		[&](float *host) { return swt_features_device(w, feature_mask, d, ls, n_lines, N, levels, band, p, host, block); });
}

// The packet entries: the nodes of `level` of a transformed packet line / image as a Band table, node f of
// the table the natural node perm(f) -- perm the identity (order 0) or the Gray code (order 1: rising frequency).
static int wp_order(int order, int f) { return order ? f ^ (f >> 1) : f; }

int dwt_hip_wp_features1d_batch(unsigned feature_mask, const void *ptr, size_t line_stride, size_t elem_stride, int n_lines, int N, int level,
	int order, float p, float *fv, size_t fv_stride)
{
	if (check_inited() || check_request(feature_mask, ptr, fv, p))
		return 1;
	if (n_lines < 0 || N < 1 || line_stride > (size_t)LONG_MAX / 2 || elem_stride > INT_MAX || fv_stride > (size_t)LONG_MAX / 8 || order < 0 || order > 1)
		return fail("packet features: bad arguments");
	if (level < 0 || (N >> level) < 1)
		return fail("packet features: level %d of a line of %d samples", level, N);
	if (level > 30 || (1 << level) > FEAT_MAX_BANDS)
		return fail("packet features: level %d has more than %d nodes", level, FEAT_MAX_BANDS);
	if (elem_stride < 4 || (n_lines > 1 && line_stride < elem_stride * (size_t)N))
		return fail("packet features: lines must be apart (line stride %zu, element stride %zu)", line_stride, elem_stride);
	const Geom ge{N, 1, N, 1};
	Band bands[FEAT_MAX_BANDS];
	const int nb = 1 << level;
	for (int f = 0; f < nb; f++) {
		int s, n;
		wp_node(N, level, wp_order(order, f), &s, &n);
		bands[f] = Band{s, 0, n, 1, level};
	}
	return features(feature_mask, ptr, (long)line_stride, n_lines, (long)elem_stride * N, (long)elem_stride, ge, bands, nb, p, Moment{}, fv,
		(long)fv_stride, true);
}

int dwt_hip_wp_features2d_batch(unsigned feature_mask, const void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y,
	int level, int order, float p, float *fv, size_t fv_stride)
{
	if (check_inited() || check_request(feature_mask, ptr, fv, p))
		return 1;
	if (batch < 0 || size_x < 1 || size_y < 1 || batch_stride > (size_t)LONG_MAX / 2 || fv_stride > (size_t)LONG_MAX / 8 || order < 0 || order > 1)
		return fail("packet features: bad arguments");
	if (level < 0 || (size_x >> level) < 1 || (size_y >> level) < 1)
		return fail("packet features: level %d of images of %d x %d", level, size_x, size_y);
	if (level > 15 || (1 << (2 * level)) > FEAT_MAX_BANDS)
		return fail("packet features: level %d has more than %d nodes", level, FEAT_MAX_BANDS);
	if (stride_x < 4l * size_x || (batch > 1 && batch_stride < (size_t)stride_x * size_y))
		return fail("packet features: images must be dense and apart (stride %d, batch stride %zu)", stride_x, batch_stride);
	const Geom ge{size_x, size_y, size_x, size_y};
	Band bands[FEAT_MAX_BANDS];
	const int nn = 1 << level;
	for (int fy = 0; fy < nn; fy++)
		for (int fx = 0; fx < nn; fx++) {
			int sx, w, sy, h;
			wp_node(size_x, level, wp_order(order, fx), &sx, &w);
			wp_node(size_y, level, wp_order(order, fy), &sy, &h);
			bands[fy * nn + fx] = Band{sx, sy, w, h, level};
		}
	return features(feature_mask, ptr, (long)batch_stride, batch, stride_x, 4, ge, bands, nn * nn, p, Moment{}, fv, (long)fv_stride, true);
}

int dwt_hip_band_feature(int feature, const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int j, float p, float *value)
{
	if (feature < 0 || feature >= DWT_HIP_FEATURE_COUNT)
		return fail("unknown feature %d", feature);
	if (check_inited() || check_request(DWT_HIP_FEATURE_BIT(feature), ptr, value, p))
		return 1;
	if (size_x <= 0 || size_y <= 0 || j < 0 || j > 30)
		return fail("bad band: %d x %d, level %d", size_x, size_y, j);
	if (size_y == 1)
		stride_x = stride_y * size_x; // (one row: its stride is never used -- the reference's spectra programs pass 0)
	const Geom ge{size_x, size_y, size_x, size_y};
	const Band band{0, 0, size_x, size_y, j};
	return features(DWT_HIP_FEATURE_BIT(feature), ptr, 0, 1, stride_x, stride_y, ge, &band, 1, p, Moment{}, value, 0, false);
}

int dwt_hip_band_moment(const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int n, int central, float c, float *value)
{
	if (check_inited())
		return 1;
	if (!ptr || !value)
		return fail("null pointer argument");
	if (size_x <= 0 || size_y <= 0)
		return fail("bad band: %d x %d", size_x, size_y);
	if (size_y == 1)
		stride_x = stride_y * size_x; // (one row: its stride is never used -- the reference's spectra programs pass 0)
	const Geom ge{size_x, size_y, size_x, size_y};
	const Band band{0, 0, size_x, size_y, 0};
	Moment mom;
	mom.use_c = !central;
	mom.c = c;
	mom.n = n;
	mom.raw = true;
	// the sum of the asked power lies in the plane of the variance (exponents outside 3, 4), the skew or the kurtosis
	const int as = n == 3 ? DWT_HIP_FEATURE_SKEW : n == 4 ? DWT_HIP_FEATURE_KURT : DWT_HIP_FEATURE_VAR;
	return features(DWT_HIP_FEATURE_BIT(as), ptr, 0, 1, stride_x, stride_y, ge, &band, 1, 2.f, mom, value, 0, false);
}

int dwt_hip_abs(void *ptr, int stride_x, int stride_y, int size_x, int size_y)
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
	if (dwt_hip_is_device_pointer(ptr))
		return check_dev_align({ptr}, {stride_x, stride_y}) || launched(launch_feat_abs(ptr, stride_x, stride_y, size_x, size_y, g.stream), "feature", "abs");
	const Frame fr{ptr, stride_x, stride_y, 4, size_x, size_y, false};
	Img A;
	if (frame_stage(fr, g.frame_a, &A) || launched(launch_feat_abs(A.p, A.sx, 4, size_x, size_y, g.stream), "feature", "abs"))
		return 1;
	return frame_unpack(fr, A.p, A.sx);
}

} // extern "C"
#pragma GCC visibility pop
