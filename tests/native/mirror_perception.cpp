// Driver of the perception half of include/tscm/tscm_calib.hpp for tests/test_gpu_cpp_mirror.py: it calls
// rectify_pair_rotation / rectify_pair_maps / stereo_match / stereo_filter / stereo_points, Panorama / exposure_gains and
// Sweep / sweep_points the way a user's program does and writes every array they return, so that the test can hold each
// against the ctypes wrappers of tscm_calib_amd on the same inputs.  C++11, the header only; needs a GPU.
//   usage: mirror_perception pair|panorama|sweep in.bin out.bin
//   exit:  0 done, 2 bad arguments or a bad input file (text on stderr), 3 a std::exception (its text on stderr)
//
// Both files are one container of named arrays, little-endian:
//   int32 magic 0x4D435354 ("TSCM"), int32 version 1, int32 n_records, then per record
//   int32 name_len, int32 type, int32 ndim, int32 dims[ndim], name_len bytes of name, prod(dims) elements of raw data
//   type: 0 uint8, 1 int16, 2 uint16, 3 int32, 4 int64, 5 float32, 6 float64
//
// pair, input:   intr f64 [2,9], Twc f64 [2,12] (row-major 3x4), img_a, img_b u8 [h,w], size i32 [2] (width, height of the
//                rectified images), cases i32 [K,2] (projection kind, 1 = also match / filter / points), fov f64 [K,2]
//                (fov_x, fov_y), stereo i32 [7] (min_disparity, num_disparities, p1, p2, paths, uniqueness_ratio,
//                disp12_max_diff), filter i32 [3] (speckle_window_size, speckle_range, median)
//       output:  rotation f64 [3,3] (rectify_pair_rotation), baseline f64 [1], and per case k (suffix _k):
//                desc f64 [2,30] (intr 9, R 9, fx fy cx cy offset_x offset_y, width height out_stride check_w2 out_offset
//                w2), mapx, mapy f32 [2,H,W], rect u8 [2,H,W] (tscm_remap); where asked: disparity, filtered i16 [H,W],
//                points, points_f f64 [H,W,3] and valid, valid_f u8 [H,W] (of the raw and of the filtered map)
// panorama, in:  intr f64 [n,9], Twc f64 [n,12], gray u8 [n,h,w], color u8 [n,h,w,3], weights u8 [n,h,w] and weight_on
//                i32 [n] (0: a NULL entry), pano i32 [2] (width, height), pad i32 [1] (bytes added to every row of the padded
//                run), configs i32 [M,5] (mode, levels, channels, 1 = with the weight images, projection kind)
//       output:  per config m (suffix _m): count, sum i64 [n,n] (stride 0) and count_p, sum_p (padded rows), gains u16 [n]
//                (exposure_gains of count, sum), out, out_g (with those gains), out_p, out_pg (padded rows) u8 [H,W,C]
// sweep, input:  intr, Twc, gray, color, pano, pad as above, inv f64 [D], params i32 [6] (num_hypotheses, p1, p2, paths,
//                uniqueness_ratio, wrap_x), gains u16 [n], configs i32 [M,3] (mode, levels, channels)
//       output:  index, index_p i16 [H,W] (depth at stride 0 and with padded rows), points f64 [H,W,3], valid u8 [H,W], and
//                per config m: null (compose with index16 = NULL), explicit (the same map passed), covered and coverage
//                (the call with a coverage vector), invalid (an all-invalid map), padg and coverage_p (padded rows, the
//                gains and a coverage vector), pano (Panorama::compose of the same mode without weights)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tscm/tscm_calib.hpp"

struct BadInput { std::string what; };

template <class T> struct Code;
template <> struct Code<unsigned char> { enum { value = 0 }; };
template <> struct Code<short> { enum { value = 1 }; };
template <> struct Code<unsigned short> { enum { value = 2 }; };
template <> struct Code<int> { enum { value = 3 }; };
template <> struct Code<long long> { enum { value = 4 }; };
template <> struct Code<float> { enum { value = 5 }; };
template <> struct Code<double> { enum { value = 6 }; };
static const size_t kTypeSize[7] = { 1, 2, 2, 4, 8, 4, 8 };

struct Record {
    std::string name;
    int type;
    std::vector<int> dims;
    std::vector<unsigned char> bytes;
    size_t count() const { size_t n = 1; for (size_t k = 0; k < dims.size(); ++k) n *= (size_t)dims[k]; return n; }
};

class Bag {
public:
    void load(const char *path)
    {
        std::ifstream f(path, std::ios::binary);
        int head[3] = { 0, 0, 0 };
        if (!f.read(reinterpret_cast<char *>(head), sizeof(head)) || head[0] != 0x4D435354 || head[1] != 1 || head[2] < 0) throw BadInput{ "not a version 1 container" };
        for (int r = 0; r < head[2]; ++r) {
            int h[3];
            Record rec;
            if (!f.read(reinterpret_cast<char *>(h), sizeof(h)) || h[0] < 1 || h[0] > 64 || h[1] < 0 || h[1] > 6 || h[2] < 0 || h[2] > 6) throw BadInput{ "a bad record header" };
            rec.type = h[1];
            rec.dims.resize((size_t)h[2]);
            if (h[2] && !f.read(reinterpret_cast<char *>(rec.dims.data()), (std::streamsize)(sizeof(int) * rec.dims.size()))) throw BadInput{ "a cut record" };
            for (size_t k = 0; k < rec.dims.size(); ++k)
                if (rec.dims[k] < 0 || rec.dims[k] > (1 << 24)) throw BadInput{ "a bad dimension" };
            if (rec.count() > ((size_t)1 << 28)) throw BadInput{ "a record too large" };
            rec.name.resize((size_t)h[0]);
            rec.bytes.resize(rec.count() * kTypeSize[rec.type]);
            if (!f.read(&rec.name[0], h[0]) || (!rec.bytes.empty() && !f.read(reinterpret_cast<char *>(rec.bytes.data()), (std::streamsize)rec.bytes.size())))
                throw BadInput{ "a cut record" };
            recs_.push_back(rec);
        }
    }
    bool save(const char *path) const
    {
        std::ofstream f(path, std::ios::binary);
        const int head[3] = { 0x4D435354, 1, (int)recs_.size() };
        f.write(reinterpret_cast<const char *>(head), sizeof(head));
        for (size_t r = 0; r < recs_.size(); ++r) {
            const Record &rec = recs_[r];
            const int h[3] = { (int)rec.name.size(), rec.type, (int)rec.dims.size() };
            f.write(reinterpret_cast<const char *>(h), sizeof(h));
            f.write(reinterpret_cast<const char *>(rec.dims.data()), (std::streamsize)(sizeof(int) * rec.dims.size()));
            f.write(rec.name.data(), (std::streamsize)rec.name.size());
            f.write(reinterpret_cast<const char *>(rec.bytes.data()), (std::streamsize)rec.bytes.size());
        }
        return (bool)f.flush();
    }
    const Record *find(const std::string &name) const
    {
        for (size_t r = 0; r < recs_.size(); ++r)
            if (recs_[r].name == name) return &recs_[r];
        return NULL;
    }
    // the record `name` of element type T and exactly these dimensions (a dimension given as -1 is free)
    template <class T> std::vector<T> get(const std::string &name, const std::vector<int> &dims, std::vector<int> *found = NULL) const
    {
        const Record *rec = find(name);
        if (!rec) throw BadInput{ "no record " + name };
        bool ok = rec->type == (int)Code<T>::value && rec->dims.size() == dims.size();
        for (size_t k = 0; ok && k < dims.size(); ++k) ok = dims[k] < 0 || dims[k] == rec->dims[k];
        if (!ok) throw BadInput{ "record " + name + " has another type or shape" };
        if (found) *found = rec->dims;
        std::vector<T> out(rec->count());
        if (!out.empty()) std::memcpy(out.data(), rec->bytes.data(), rec->bytes.size());
        return out;
    }
    template <class T> void put(const std::string &name, const std::vector<int> &dims, const T *data)
    {
        Record rec;
        rec.name = name; rec.type = (int)Code<T>::value; rec.dims = dims;
        rec.bytes.resize(rec.count() * sizeof(T));
        if (!rec.bytes.empty()) std::memcpy(rec.bytes.data(), data, rec.bytes.size());
        recs_.push_back(rec);
    }

private:
    std::vector<Record> recs_;
};

static std::vector<int> shape(int a) { return std::vector<int>(1, a); }
static std::vector<int> shape(int a, int b) { std::vector<int> d(2); d[0] = a; d[1] = b; return d; }
static std::vector<int> shape(int a, int b, int c) { std::vector<int> d = shape(a, b); d.push_back(c); return d; }
static std::vector<int> shape(int a, int b, int c, int e) { std::vector<int> d = shape(a, b, c); d.push_back(e); return d; }

static std::string tag(const char *name, int k)
{
    std::ostringstream s;
    s << name << "_" << k;
    return s.str();
}

// n images of `rows` rows of `row` bytes each, copied into rows of row + pad bytes; the padding holds other values
static std::vector<std::vector<unsigned char> > padded(const std::vector<unsigned char> &all, int n, int rows, int row, int pad)
{
    std::vector<std::vector<unsigned char> > out((size_t)n);
    for (int k = 0; k < n; ++k) {
        out[(size_t)k].assign((size_t)rows * (row + pad), 0);
        for (int i = 0; i < rows; ++i) {
            unsigned char *dst = &out[(size_t)k][(size_t)i * (row + pad)];
            std::memcpy(dst, &all[((size_t)k * rows + i) * row], (size_t)row);
            for (int b = 0; b < pad; ++b) dst[row + b] = (unsigned char)(0xE1 + 7 * b + 3 * i);
        }
    }
    return out;
}

static std::vector<const unsigned char *> pointers(const std::vector<unsigned char> &all, int n, size_t each)
{
    std::vector<const unsigned char *> p((size_t)n);
    for (int k = 0; k < n; ++k) p[(size_t)k] = all.data() + (size_t)k * each;
    return p;
}

static std::vector<const unsigned char *> pointers(const std::vector<std::vector<unsigned char> > &imgs)
{
    std::vector<const unsigned char *> p(imgs.size());
    for (size_t k = 0; k < imgs.size(); ++k) p[k] = imgs[k].data();
    return p;
}

static void put_desc(Bag &out, const std::string &name, const tscm_map_desc desc[2])
{
    std::vector<double> v;
    for (int k = 0; k < 2; ++k) {
        const tscm_map_desc &d = desc[k];
        v.insert(v.end(), d.intr, d.intr + 9);
        v.insert(v.end(), d.R, d.R + 9);
        const double tail[12] = { d.fx, d.fy, d.cx, d.cy, d.offset_x, d.offset_y, (double)d.width, (double)d.height, (double)d.out_stride, (double)d.check_w2,
                                  (double)d.out_offset, d.w2 };
        v.insert(v.end(), tail, tail + 12);
    }
    out.put(name, shape(2, 30), v.data());
}

static void run_pair(const Bag &in, Bag &out)
{
    const std::vector<double> intr = in.get<double>("intr", shape(2, 9)), Twc = in.get<double>("Twc", shape(2, 12));
    std::vector<int> src;
    const std::vector<unsigned char> img_a = in.get<unsigned char>("img_a", shape(-1, -1), &src);
    const std::vector<unsigned char> img_b = in.get<unsigned char>("img_b", src);
    const std::vector<int> size = in.get<int>("size", shape(2));
    std::vector<int> kdim;
    const std::vector<int> cases = in.get<int>("cases", shape(-1, 2), &kdim);
    const std::vector<double> fov = in.get<double>("fov", shape(kdim[0], 2));
    const std::vector<int> sp = in.get<int>("stereo", shape(7)), fp = in.get<int>("filter", shape(3));
    if (size[0] < 1 || size[1] < 1 || src[0] < 1 || src[1] < 1) throw BadInput{ "an empty image" };
    const tscm::Size rsize = { size[0], size[1] };
    const int W = size[0], H = size[1], w = src[1], h = src[0];

    const double *Ta = &Twc[0], *Tb = &Twc[12];
    const double ta[3] = { Ta[3], Ta[7], Ta[11] }, tb[3] = { Tb[3], Tb[7], Tb[11] };
    const tscm::Mat33 Rp = tscm::rectify_pair_rotation(ta, tb);
    out.put("rotation", shape(3, 3), Rp.a);
    const double dt[3] = { tb[0] - ta[0], tb[1] - ta[1], tb[2] - ta[2] };
    const double baseline = std::sqrt(dt[0] * dt[0] + dt[1] * dt[1] + dt[2] * dt[2]);
    out.put("baseline", shape(1), &baseline);

    for (int k = 0; k < kdim[0]; ++k) {
        const int kind = cases[2 * (size_t)k];
        tscm_map_desc desc[2];
        std::vector<float> mapx[2], mapy[2];
        tscm::rectify_pair_maps(&intr[0], Ta, &intr[9], Tb, kind, rsize, fov[2 * (size_t)k], fov[2 * (size_t)k + 1], desc, mapx, mapy);
        put_desc(out, tag("desc", k), desc);
        std::vector<float> mx(mapx[0]), my(mapy[0]);
        mx.insert(mx.end(), mapx[1].begin(), mapx[1].end());
        my.insert(my.end(), mapy[1].begin(), mapy[1].end());
        out.put(tag("mapx", k), shape(2, H, W), mx.data());
        out.put(tag("mapy", k), shape(2, H, W), my.data());
        std::vector<unsigned char> rect((size_t)2 * W * H, 0);
        for (int c = 0; c < 2; ++c)
            tscm::check(tscm_remap((c ? img_b : img_a).data(), w, h, w, 1, mapx[c].data(), mapy[c].data(), W, H, W, 0, 0, &rect[(size_t)c * W * H], W));
        out.put(tag("rect", k), shape(2, H, W), rect.data());
        if (!cases[2 * (size_t)k + 1]) continue;

        tscm_stereo_params params;
        tscm_stereo_default_params(&params);
        params.min_disparity = sp[0]; params.num_disparities = sp[1]; params.p1 = sp[2]; params.p2 = sp[3];
        params.paths = sp[4]; params.uniqueness_ratio = sp[5]; params.disp12_max_diff = sp[6];
        const std::vector<short> disparity = tscm::stereo_match(&rect[0], &rect[(size_t)W * H], rsize, &params);
        tscm_stereo_filter_params post;
        tscm_stereo_filter_default_params(&post);
        post.min_disparity = params.min_disparity;
        post.speckle_window_size = fp[0]; post.speckle_range = fp[1]; post.median = fp[2];
        const std::vector<short> filtered = tscm::stereo_filter(disparity, rsize, &post);
        out.put(tag("disparity", k), shape(H, W), disparity.data());
        out.put(tag("filtered", k), shape(H, W), filtered.data());
        for (int f = 0; f < 2; ++f) {
            std::vector<unsigned char> valid;
            const std::vector<tscm::Point3d> pts = tscm::stereo_points(f ? filtered : disparity, rsize, params.min_disparity, desc[0], kind, baseline, valid);
            out.put(tag(f ? "points_f" : "points", k), shape(H, W, 3), &pts[0].x);
            out.put(tag(f ? "valid_f" : "valid", k), shape(H, W), valid.data());
        }
    }
}

// what the panorama and the sweep run share: the rig, its frame in grey and in colour, padded copies of both
struct Frame {
    int n, w, h, pad;
    tscm::Size image, pano;
    std::vector<double> intr, Twc;
    std::vector<unsigned char> gray, color;
    std::vector<std::vector<unsigned char> > gray_pad, color_pad;

    explicit Frame(const Bag &in)
    {
        std::vector<int> d;
        gray = in.get<unsigned char>("gray", shape(-1, -1, -1), &d);
        n = d[0]; h = d[1]; w = d[2];
        if (n < 1 || h < 1 || w < 1) throw BadInput{ "an empty frame" };
        color = in.get<unsigned char>("color", shape(n, h, w, 3));
        intr = in.get<double>("intr", shape(n, 9));
        Twc = in.get<double>("Twc", shape(n, 12));
        const std::vector<int> p = in.get<int>("pano", shape(2));
        pad = in.get<int>("pad", shape(1))[0];
        if (p[0] < 1 || p[1] < 1 || pad < 1 || pad > 64) throw BadInput{ "pano or pad out of range" };
        image.width = w; image.height = h;
        pano.width = p[0]; pano.height = p[1];
        gray_pad = padded(gray, n, h, w, pad);
        color_pad = padded(color, n, h, 3 * w, pad);
    }
    std::vector<const unsigned char *> plain(int channels) const { return pointers(channels == 3 ? color : gray, n, (size_t)w * h * channels); }
    std::vector<const unsigned char *> wide(int channels) const { return pointers(channels == 3 ? color_pad : gray_pad); }
    int wide_stride(int channels) const { return w * channels + pad; }
};

static void run_panorama(const Bag &in, Bag &out)
{
    const Frame fr(in);
    const int n = fr.n;
    const std::vector<unsigned char> weights = in.get<unsigned char>("weights", shape(n, fr.h, fr.w));
    const std::vector<int> weight_on = in.get<int>("weight_on", shape(n));
    std::vector<const unsigned char *> wptr = pointers(weights, n, (size_t)fr.w * fr.h);
    for (int k = 0; k < n; ++k)
        if (!weight_on[(size_t)k]) wptr[(size_t)k] = NULL;
    std::vector<int> mdim;
    const std::vector<int> configs = in.get<int>("configs", shape(-1, 5), &mdim);
    for (int m = 0; m < mdim[0]; ++m) {
        const int *cfg = &configs[5 * (size_t)m];
        const int channels = cfg[2];
        if (channels != 1 && channels != 3) throw BadInput{ "channels are 1 or 3" };
        tscm_panorama_params params;
        tscm_panorama_default_params(&params);
        params.mode = cfg[0]; params.levels = cfg[1];
        tscm::Panorama p(n, fr.intr.data(), fr.Twc.data(), fr.image, channels, fr.pano, &params, cfg[3] ? wptr.data() : NULL, cfg[4]);
        const std::vector<const unsigned char *> plain = fr.plain(channels), wide = fr.wide(channels);
        const int stride = fr.wide_stride(channels);
        std::vector<long long> count, sum, count_p, sum_p;
        p.overlap(plain.data(), 0, count, sum);
        p.overlap(wide.data(), stride, count_p, sum_p);
        const std::vector<unsigned short> gains = tscm::exposure_gains(n, count, sum);
        out.put(tag("count", m), shape(n, n), count.data());
        out.put(tag("sum", m), shape(n, n), sum.data());
        out.put(tag("count_p", m), shape(n, n), count_p.data());
        out.put(tag("sum_p", m), shape(n, n), sum_p.data());
        out.put(tag("gains", m), shape(n), gains.data());
        const std::vector<int> oshape = shape(fr.pano.height, fr.pano.width, channels);
        out.put(tag("out", m), oshape, p.compose(plain.data()).data());
        out.put(tag("out_g", m), oshape, p.compose(plain.data(), 0, gains.data()).data());
        out.put(tag("out_p", m), oshape, p.compose(wide.data(), stride).data());
        out.put(tag("out_pg", m), oshape, p.compose(wide.data(), stride, gains.data()).data());
    }
}

static void run_sweep(const Bag &in, Bag &out)
{
    const Frame fr(in);
    const int n = fr.n, W = fr.pano.width, H = fr.pano.height;
    std::vector<int> ddim;
    const std::vector<double> inv = in.get<double>("inv", shape(-1), &ddim);
    const std::vector<int> sp = in.get<int>("params", shape(6));
    const std::vector<unsigned short> gains = in.get<unsigned short>("gains", shape(n));
    std::vector<int> mdim;
    const std::vector<int> configs = in.get<int>("configs", shape(-1, 3), &mdim);
    tscm_sweep_params params;
    tscm_sweep_default_params(&params);
    params.num_hypotheses = sp[0]; params.p1 = sp[1]; params.p2 = sp[2]; params.paths = sp[3]; params.uniqueness_ratio = sp[4]; params.wrap_x = sp[5];
    tscm::Sweep sweep(n, fr.intr.data(), fr.Twc.data(), fr.image, fr.pano, inv, &params);

    const std::vector<short> index = sweep.depth(fr.plain(1).data());
    const std::vector<short> index_p = sweep.depth(fr.wide(1).data(), fr.wide_stride(1));
    out.put("index", shape(H, W), index.data());
    out.put("index_p", shape(H, W), index_p.data());
    std::vector<unsigned char> valid;
    const std::vector<tscm::Point3d> pts = sweep.points(index, valid);
    out.put("points", shape(H, W, 3), &pts[0].x);
    out.put("valid", shape(H, W), valid.data());

    const std::vector<short> nothing(index.size(), (short)-16);
    for (int m = 0; m < mdim[0]; ++m) {
        const int *cfg = &configs[3 * (size_t)m];
        const int channels = cfg[2];
        if (channels != 1 && channels != 3) throw BadInput{ "channels are 1 or 3" };
        tscm_sweep_compose_params blend;
        tscm_sweep_compose_default_params(&blend);
        blend.mode = cfg[0]; blend.levels = cfg[1];
        const std::vector<const unsigned char *> plain = fr.plain(channels), wide = fr.wide(channels);
        const std::vector<int> oshape = shape(H, W, channels);
        std::vector<unsigned char> coverage, coverage_p;
        out.put(tag("null", m), oshape, sweep.compose(plain.data(), channels, NULL, &blend).data());
        out.put(tag("explicit", m), oshape, sweep.compose(plain.data(), channels, &index, &blend).data());
        out.put(tag("covered", m), oshape, sweep.compose(plain.data(), channels, &index, &blend, NULL, 0, &coverage).data());
        out.put(tag("coverage", m), shape(H, W), coverage.data());
        out.put(tag("invalid", m), oshape, sweep.compose(plain.data(), channels, &nothing, &blend).data());
        out.put(tag("padg", m), oshape, sweep.compose(wide.data(), channels, &index, &blend, gains.data(), fr.wide_stride(channels), &coverage_p).data());
        out.put(tag("coverage_p", m), shape(H, W), coverage_p.data());
        tscm_panorama_params pp;
        tscm_panorama_default_params(&pp);
        pp.mode = cfg[0]; pp.levels = cfg[1];
        tscm::Panorama pano(n, fr.intr.data(), fr.Twc.data(), fr.image, channels, fr.pano, &pp);
        out.put(tag("pano", m), oshape, pano.compose(plain.data()).data());
    }
}

int main(int argc, char **argv)
{
    const std::string task = argc == 4 ? argv[1] : "";
    if (task != "pair" && task != "panorama" && task != "sweep") {
        std::fprintf(stderr, "usage: %s pair|panorama|sweep in.bin out.bin\n", argv[0]);
        return 2;
    }
    try {
        Bag in, out;
        in.load(argv[2]);
        if (task == "pair") run_pair(in, out);
        else if (task == "panorama") run_panorama(in, out);
        else run_sweep(in, out);
        if (!out.save(argv[3])) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    } catch (const BadInput &e) {
        std::fprintf(stderr, "%s: %s\n", argv[2], e.what.c_str());
        return 2;
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 3;
    }
    return 0;
}
