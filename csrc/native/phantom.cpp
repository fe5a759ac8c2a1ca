#include "phantom.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace sart {

const char* const kPhantomScoreNames[kPhantomScoreCount] = {"rel_l2",     "cosine",    "total_ratio",
                                                            "peak_ratio", "max_error", "inside_fraction"};

namespace {

double ratio(double num, double den) { return den == 0.0 ? std::numeric_limits<double>::quiet_NaN() : num / den; }

}  // namespace

PhantomScores phantom_scores(const double s[kPhantomSumCount]) {
    PhantomScores r;
    r.rel_l2 = std::sqrt(ratio(s[kSumDD], s[kSumTT]));
    const double norms = std::sqrt(s[kSumXX] * s[kSumTT]);
    r.cosine = ratio(s[kSumXT], norms);
    r.total_ratio = ratio(s[kSumX], s[kSumT]);
    r.peak_ratio = ratio(s[kMaxX], s[kMaxT]);
    r.max_error = ratio(s[kMaxD], s[kMaxT]);
    r.inside_fraction = ratio(s[kSumIn], s[kSumX]);
    return r;
}

#ifdef SART_HAVE_HDF5

namespace {

constexpr uint64_t kCheckBytes = 32ull << 20;  // rows validated per read: about this many bytes

void read_value_rows(hid_t ds, const std::string& filename, uint64_t k0, uint64_t n, uint64_t nvoxel, double* out) {
    if (n == 0) return;
    H5Id fsp(H5Dget_space(ds), H5Id::kSpace);
    hsize_t o[2] = {k0, 0}, c[2] = {n, nvoxel};
    H5Id msp(H5Screate_simple(2, c, nullptr), H5Id::kSpace);
    if (H5Sselect_hyperslab(fsp, H5S_SELECT_SET, o, nullptr, c, nullptr) < 0 ||
        H5Dread(ds, H5T_NATIVE_DOUBLE, msp, fsp, H5P_DEFAULT, out) < 0)
        throw Error("Unable to read phantom/value of " + filename + ".");
}

void create_sized(hid_t grp, const char* name, hid_t ftype, const std::vector<hsize_t>& dims) {
    H5Id sp(H5Screate_simple((int)dims.size(), dims.data(), nullptr), H5Id::kSpace);
    H5Id ds(H5Dcreate2(grp, name, ftype, sp, H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT), H5Id::kDataset);
    if (!ds.valid()) throw Error(std::string("Unable to create dataset phantom/") + name + ".");
}

}  // namespace

PhantomFile::PhantomFile(const std::string& filename, uint64_t nvoxel) : filename_(filename), nvox_(nvoxel) {
    SART_H5_LOCK;
    H5Id f = h5_open_file(filename_);
    if (!h5_exists(f, "phantom/value")) throw Error("Phantom file " + filename_ + " has no dataset phantom/value.");
    H5Id ds = h5_open_dataset(f, "phantom/value");
    const H5T_class_t cls = [&] {
        H5Id t(H5Dget_type(ds), H5Id::kType);
        return H5Tget_class(t);
    }();
    const std::vector<hsize_t> dims = h5_dims(ds);
    if (cls != H5T_FLOAT || dims.size() != 2)
        throw Error("Dataset phantom/value of " + filename_ + " must be a [n][nvoxel] array of fp32 or fp64 values.");
    if (dims[1] != nvox_)
        throw Error("Dataset phantom/value of " + filename_ + " has " + std::to_string(dims[1]) +
                    " voxels per row, the RTM has " + std::to_string(nvox_) + ".");
    n_ = dims[0];
    if (n_ == 0) throw Error("Dataset phantom/value of " + filename_ + " holds no phantom (n = 0).");
    const uint64_t step = std::max<uint64_t>(1, kCheckBytes / (nvox_ * sizeof(double)));
    std::vector<double> rows((size_t)(std::min(step, n_) * nvox_));
    for (uint64_t k0 = 0; k0 < n_; k0 += step) {
        const uint64_t n = std::min(step, n_ - k0);
        read_value_rows(ds, filename_, k0, n, nvox_, rows.data());
        for (uint64_t i = 0; i < n * nvox_; ++i)
            if (!(std::isfinite(rows[i]) && rows[i] >= 0.0))
                throw Error("Dataset phantom/value of " + filename_ + " holds a negative or non-finite entry (row " +
                            std::to_string(k0 + i / nvox_) + ", voxel " + std::to_string(i % nvox_) + ").");
    }
    if (h5_exists(f, "phantom/time")) {
        time_ = h5_read_f64(f, "phantom/time");
        H5Id dt = h5_open_dataset(f, "phantom/time");
        if (h5_dims(dt).size() != 1 || time_.size() != n_)
            throw Error("Dataset phantom/time of " + filename_ + " must hold one time per phantom (" +
                        std::to_string(n_) + ").");
        for (uint64_t k = 0; k < n_; ++k)
            if (!std::isfinite(time_[k]) || (k > 0 && !(time_[k] > time_[k - 1])))
                throw Error("Dataset phantom/time of " + filename_ + " must be finite and strictly increasing.");
    } else {
        time_.resize(n_);
        for (uint64_t k = 0; k < n_; ++k) time_[k] = (double)k;
    }
}

void PhantomFile::read_rows(uint64_t k0, uint64_t n, double* out) const {
    if (k0 + n > n_) throw Error("Phantom rows beyond phantom/value of " + filename_ + ".");
    SART_H5_LOCK;
    H5Id f = h5_open_file(filename_);
    H5Id ds = h5_open_dataset(f, "phantom/value");
    read_value_rows(ds, filename_, k0, n, nvox_, out);
}

void write_phantom_file(const std::string& filename, const double* value, uint64_t n, uint64_t nvoxel,
                        const double* time, bool as_f32) {
    SART_H5_LOCK;
    H5Id f = h5_create_file(filename);
    H5Id g = h5_create_group(f, "phantom");
    H5Id ds = h5_create_dataset(g, "value", {n, nvoxel}, as_f32 ? H5T_IEEE_F32LE : H5T_IEEE_F64LE);
    h5_write_box(ds, {0, 0}, {n, nvoxel}, H5T_NATIVE_DOUBLE, value);
    if (time) {
        H5Id dt = h5_create_dataset(g, "time", {n}, H5T_IEEE_F64LE);
        h5_write_box(dt, {0}, {n}, H5T_NATIVE_DOUBLE, time);
    }
}

PhantomWriter::PhantomWriter(const std::string& filename, uint64_t n, uint64_t nc, uint64_t npixel,
                             const std::string& source, const double* time, bool into_existing)
    : filename_(filename), n_(n), nc_(nc), npix_(npixel) {
    if (n_ == 0 || nc_ == 0 || npix_ == 0) throw Error("A phantom group needs phantoms, columns and pixels.");
    SART_H5_LOCK;
    H5Id f = into_existing ? h5_open_file(filename_, true) : h5_create_file(filename_);
    H5Id g = h5_create_group(f, "phantom");
    h5_write_attr_string(g, "file", source);
    h5_write_f64(g, "time", {n_}, time);
    create_sized(g, "image", H5T_IEEE_F64LE, {n_, npix_});
    create_sized(g, "sums", H5T_IEEE_F64LE, {n_, nc_, (hsize_t)kPhantomSumCount});
    for (const char* name : kPhantomScoreNames) create_sized(g, name, H5T_IEEE_F64LE, {n_, nc_});
    create_sized(g, "status", H5T_STD_I32LE, {n_, nc_});
    create_sized(g, "iterations", H5T_STD_I32LE, {n_, nc_});
}

void PhantomWriter::write_phantom(uint64_t k, const double* sums, const int32_t* status, const int32_t* iterations) {
    if (k >= n_) throw Error("Phantom " + std::to_string(k) + " is out of bounds.");
    std::vector<double> score((size_t)kPhantomScoreCount * nc_);
    for (uint64_t c = 0; c < nc_; ++c) {
        const PhantomScores s = phantom_scores(sums + c * kPhantomSumCount);
        const double v[kPhantomScoreCount] = {s.rel_l2,     s.cosine,    s.total_ratio,
                                              s.peak_ratio, s.max_error, s.inside_fraction};
        for (int i = 0; i < kPhantomScoreCount; ++i) score[(size_t)i * nc_ + c] = v[i];
    }
    SART_H5_LOCK;
    H5Id f = h5_open_file(filename_, true);
    auto put = [&](const char* name, const std::vector<uint64_t>& off, const std::vector<uint64_t>& cnt, hid_t mtype,
                   const void* data) {
        H5Id ds = h5_open_dataset(f, std::string("phantom/") + name);
        h5_write_box(ds, off, cnt, mtype, data);
    };
    put("sums", {k, 0, 0}, {1, nc_, (uint64_t)kPhantomSumCount}, H5T_NATIVE_DOUBLE, sums);
    for (int i = 0; i < kPhantomScoreCount; ++i)
        put(kPhantomScoreNames[i], {k, 0}, {1, nc_}, H5T_NATIVE_DOUBLE, score.data() + (size_t)i * nc_);
    put("status", {k, 0}, {1, nc_}, H5T_NATIVE_INT32, status);
    put("iterations", {k, 0}, {1, nc_}, H5T_NATIVE_INT32, iterations);
}

void PhantomWriter::write_images(const double* image) {
    SART_H5_LOCK;
    H5Id f = h5_open_file(filename_, true);
    H5Id ds = h5_open_dataset(f, "phantom/image");
    h5_write_box(ds, {0, 0}, {n_, npix_}, H5T_NATIVE_DOUBLE, image);
}

#endif  // SART_HAVE_HDF5

}  // namespace sart
