#include "holdout.hpp"

#include <cmath>
#include <limits>

#include "../kernels/philox.hpp"

namespace sart {

void holdout_pixel_folds(uint64_t seed, int K, uint64_t pixel0, uint64_t n, int32_t* out) {
    if (K < 2 || K > 32) throw Error("Hold-out folds must be within 2 .. 32, " + std::to_string(K) + " given.");
    if (pixel0 + n > (uint64_t)1 << 32) throw Error("Hold-out folds apply to fewer than 2^32 pixels.");
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (uint64_t i = 0; i < n; ++i) {
        const Philox4 w = philox4x32_10((uint32_t)(pixel0 + i), 0u, kHoldoutCounterTag, 0u, k0, k1);
        out[i] = (int32_t)(((uint64_t)w.w[0] * (uint64_t)K) >> 32);
    }
}

void holdout_camera_folds(const int64_t* camera_pixels, int ncam, uint64_t pixel0, uint64_t n, int32_t* out) {
    uint64_t start = 0, i = 0;
    for (int m = 0; m < ncam && i < n; ++m) {
        if (camera_pixels[m] < 0) throw Error("A camera cannot hold a negative number of pixels.");
        const uint64_t end = start + (uint64_t)camera_pixels[m];
        for (; i < n && pixel0 + i < end; ++i) out[i] = (int32_t)m;
        start = end;
    }
    if (i < n) throw Error("Hold-out folds: pixels beyond the cameras' pixels.");
}

void holdout_mask(const double* g, const int32_t* fold, int64_t n, int held, double* out) {
    for (int64_t p = 0; p < n; ++p) out[p] = (held >= 0 && fold[p] == held && g[p] >= 0.0) ? -1.0 : g[p];
}

int holdout_fallback(const double* betas, int nb, double beta) {
    int fallback = 0;
    for (int i = 1; i < nb; ++i)
        if (std::abs(betas[i] - beta) < std::abs(betas[fallback] - beta)) fallback = i;
    return fallback;
}

namespace {

double rms(double num, double den) {
    return den == 0.0 ? std::numeric_limits<double>::quiet_NaN() : std::sqrt(num / den);
}

}  // namespace

HoldoutScores holdout_scores(const double* sums, const uint8_t* ok, int nb, int K, int ncam, int fallback) {
    if (nb < 1 || K < 1 || ncam < 1) throw Error("Hold-out scores need weights, folds and cameras.");
    constexpr int Q = kHoldoutSumCount;
    const int nc = K + 1;
    HoldoutScores r;
    r.cv_error.resize((size_t)nb), r.cv_relative.resize((size_t)nb), r.train_error.resize((size_t)nb);
    r.cv_error_camera.resize((size_t)nb * ncam);
    r.eligible.resize((size_t)nb);
    for (int i = 0; i < nb; ++i) {
        const double* s = sums + (size_t)i * nc * ncam * Q;
        double num = 0.0, norm = 0.0, count = 0.0;
        for (int c = 1; c <= K; ++c)
            for (int m = 0; m < ncam; ++m) {
                const double* v = s + ((size_t)c * ncam + m) * Q;
                num += v[0], norm += v[1], count += v[2];
            }
        r.cv_error[i] = rms(num, count);
        r.cv_relative[i] = rms(num, norm);
        for (int m = 0; m < ncam; ++m) {
            double cnum = 0.0, ccount = 0.0;
            for (int c = 1; c <= K; ++c) {
                const double* v = s + ((size_t)c * ncam + m) * Q;
                cnum += v[0], ccount += v[2];
            }
            r.cv_error_camera[(size_t)i * ncam + m] = rms(cnum, ccount);
        }
        double tnum = 0.0, tcount = 0.0;
        for (int m = 0; m < ncam; ++m) tnum += s[(size_t)m * Q + 3], tcount += s[(size_t)m * Q + 5];
        r.train_error[i] = rms(tnum, tcount);
        bool all_ok = true;
        for (int c = 0; c < nc; ++c) all_ok = all_ok && ok[(size_t)i * nc + c] != 0;
        r.eligible[i] = (all_ok && std::isfinite(r.cv_error[i])) ? 1 : 0;
    }
    r.selected = fallback, r.found = 0;
    for (int i = 0; i < nb; ++i) {
        if (!r.eligible[i]) continue;
        if (!r.found || r.cv_error[i] < r.cv_error[r.selected]) r.selected = i;  // strictly: ties stay with the first
        r.found = 1;
    }
    return r;
}

#ifdef SART_HAVE_HDF5

namespace {

void create_holdout(hid_t grp, const char* name, hid_t ftype, const std::vector<hsize_t>& dims, bool chunk_rows) {
    H5Id sp(H5Screate_simple((int)dims.size(), dims.data(), nullptr), H5Id::kSpace);
    H5Id pl(H5Pcreate(H5P_DATASET_CREATE), H5Id::kPlist);
    bool empty = false;
    for (hsize_t d : dims) empty = empty || d == 0;
    if (chunk_rows && !empty) {  // one solution per chunk: columns arrive one at a time
        std::vector<hsize_t> ch(dims.size(), 1);
        ch.back() = dims.back();
        H5Pset_chunk(pl, (int)ch.size(), ch.data());
    }
    H5Id ds(H5Dcreate2(grp, name, ftype, sp, H5P_DEFAULT, pl, H5P_DEFAULT), H5Id::kDataset);
    if (!ds.valid()) throw Error(std::string("Unable to create dataset holdout/") + name + ".");
}

// a scalar dataset holding a fixed-length string
void write_string(hid_t grp, const char* name, const std::string& text) {
    H5Id type(H5Tcopy(H5T_C_S1), H5Id::kType);
    H5Tset_size(type, text.size());
    H5Tset_strpad(type, H5T_STR_NULLPAD);
    H5Id sp(H5Screate(H5S_SCALAR), H5Id::kSpace);
    H5Id ds(H5Dcreate2(grp, name, type, sp, H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT), H5Id::kDataset);
    if (!ds.valid() || H5Dwrite(ds, type, H5S_ALL, H5S_ALL, H5P_DEFAULT, text.data()) < 0)
        throw Error(std::string("Unable to write dataset holdout/") + name + ".");
}

}  // namespace

HoldoutWriter::HoldoutWriter(const std::string& filename, uint64_t frames, uint64_t nb, uint64_t K, uint64_t ncam,
                             uint64_t nvoxel, bool cameras, const int32_t* folds, uint64_t npixel, uint64_t seed,
                             const double* beta)
    : filename_(filename), frames_(frames), nb_(nb), nc_(K + 1), ncam_(ncam), nvox_(nvoxel) {
    if (nvox_ == 0) throw Error("Argument nvoxel must be positive.");
    if (nb_ == 0 || K == 0 || ncam_ == 0 || npixel == 0)
        throw Error("A hold-out group needs weights, folds, cameras and pixels.");
    SART_H5_LOCK;
    file_ = h5_create_file(filename_);
    H5Id g = h5_create_group(file_, "holdout");
    write_string(g, "mode", cameras ? "cameras" : "pixels");
    h5_write_i32(g, "folds", {npixel}, folds);
    h5_write_u64(g, "seed", {1}, &seed);
    h5_write_f64(g, "beta", {nb_}, beta);
    create_holdout(g, "value", H5T_IEEE_F64LE, {frames_, nb_, nc_, nvox_}, true);
    create_holdout(g, "status", H5T_STD_I32LE, {frames_, nb_, nc_}, false);
    create_holdout(g, "iterations", H5T_STD_I32LE, {frames_, nb_, nc_}, false);
    create_holdout(g, "sums", H5T_IEEE_F64LE, {frames_, nb_, nc_, ncam_, (hsize_t)kHoldoutSumCount}, false);
    for (const char* name : {"cv_error", "cv_relative", "train_error"})
        create_holdout(g, name, H5T_IEEE_F64LE, {frames_, nb_}, false);
    create_holdout(g, "cv_error_camera", H5T_IEEE_F64LE, {frames_, nb_, ncam_}, false);
    create_holdout(g, "eligible", H5T_STD_U8LE, {frames_, nb_}, false);
    create_holdout(g, "selected", H5T_STD_I32LE, {frames_}, false);
    create_holdout(g, "found", H5T_STD_U8LE, {frames_}, false);
}

hid_t HoldoutWriter::file() {
    if (!file_.valid()) file_ = h5_open_file(filename_, true);
    return file_;
}

void HoldoutWriter::close() {
    SART_H5_LOCK;
    file_.reset();
}

void HoldoutWriter::write_column(uint64_t k, uint64_t i, uint64_t c, const double* x, int32_t status,
                                 int32_t iterations) {
    if (k >= frames_ || i >= nb_ || c >= nc_)
        throw Error("Hold-out column " + std::to_string(k) + ", " + std::to_string(i) + ", " + std::to_string(c) +
                    " is out of bounds.");
    SART_H5_LOCK;
    const hid_t f = file();
    {
        H5Id ds = h5_open_dataset(f, "holdout/value");
        h5_write_box(ds, {k, i, c, 0}, {1, 1, 1, nvox_}, H5T_NATIVE_DOUBLE, x);
    }
    {
        H5Id ds = h5_open_dataset(f, "holdout/status");
        h5_write_box(ds, {k, i, c}, {1, 1, 1}, H5T_NATIVE_INT32, &status);
    }
    H5Id ds = h5_open_dataset(f, "holdout/iterations");
    h5_write_box(ds, {k, i, c}, {1, 1, 1}, H5T_NATIVE_INT32, &iterations);
}

void HoldoutWriter::read_columns(uint64_t j0, uint64_t n, double* out) {
    if (j0 + n > frames_ * nb_ * nc_) throw Error("Hold-out rows beyond the stored columns.");
    SART_H5_LOCK;
    H5Id ds = h5_open_dataset(file(), "holdout/value");
    H5Id fsp(H5Dget_space(ds), H5Id::kSpace);
    hsize_t m = nvox_;
    H5Id msp(H5Screate_simple(1, &m, nullptr), H5Id::kSpace);
    for (uint64_t j = j0; j < j0 + n; ++j) {  // a group may straddle two ladder entries: one column at a time
        hsize_t o[4] = {j / (nb_ * nc_), j / nc_ % nb_, j % nc_, 0}, c[4] = {1, 1, 1, nvox_};
        H5Sselect_hyperslab(fsp, H5S_SELECT_SET, o, nullptr, c, nullptr);
        if (H5Dread(ds, H5T_NATIVE_DOUBLE, msp, fsp, H5P_DEFAULT, out + (j - j0) * nvox_) < 0)
            throw Error("Unable to read holdout/value of " + filename_ + ".");
    }
}

void HoldoutWriter::write_frame(uint64_t k, const double* sums, const HoldoutScores& s) {
    if (k >= frames_) throw Error("Hold-out frame " + std::to_string(k) + " is out of bounds.");
    if (s.cv_error.size() != nb_ || s.cv_error_camera.size() != nb_ * ncam_ || s.eligible.size() != nb_)
        throw Error("Hold-out scores do not match the group's shape.");
    SART_H5_LOCK;
    const hid_t f = file();
    auto put = [&](const char* name, const std::vector<uint64_t>& off, const std::vector<uint64_t>& cnt, hid_t mtype,
                   const void* data) {
        H5Id ds = h5_open_dataset(f, std::string("holdout/") + name);
        h5_write_box(ds, off, cnt, mtype, data);
    };
    put("sums", {k, 0, 0, 0, 0}, {1, nb_, nc_, ncam_, (uint64_t)kHoldoutSumCount}, H5T_NATIVE_DOUBLE, sums);
    put("cv_error", {k, 0}, {1, nb_}, H5T_NATIVE_DOUBLE, s.cv_error.data());
    put("cv_relative", {k, 0}, {1, nb_}, H5T_NATIVE_DOUBLE, s.cv_relative.data());
    put("train_error", {k, 0}, {1, nb_}, H5T_NATIVE_DOUBLE, s.train_error.data());
    put("cv_error_camera", {k, 0, 0}, {1, nb_, ncam_}, H5T_NATIVE_DOUBLE, s.cv_error_camera.data());
    put("eligible", {k, 0}, {1, nb_}, H5T_NATIVE_UINT8, s.eligible.data());
    put("selected", {k}, {1}, H5T_NATIVE_INT32, &s.selected);
    put("found", {k}, {1}, H5T_NATIVE_UINT8, &s.found);
}

#endif  // SART_HAVE_HDF5

}  // namespace sart
