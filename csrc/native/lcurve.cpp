#include "lcurve.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>

namespace sart {

LcurveCorner lcurve_corner(const double* rho, const double* eta, const uint8_t* ok, int nb, int fallback) {
    LcurveCorner out;
    out.curvature.assign((size_t)std::max(nb, 0), std::numeric_limits<double>::quiet_NaN());
    out.selected = fallback;
    std::vector<int> valid;
    std::vector<double> px, py;
    for (int i = 0; i < nb; ++i) {
        if (!ok[i] || !std::isfinite(rho[i]) || !std::isfinite(eta[i]) || !(rho[i] > 0) || !(eta[i] > 0)) continue;
        valid.push_back(i);
        px.push_back(std::log(rho[i]));
        py.push_back(std::log(eta[i]));
    }
    double best = 0.0;
    for (size_t m = 1; m + 1 < valid.size(); ++m) {  // a, b, c: nearest valid neighbours
        const double abx = px[m] - px[m - 1], aby = py[m] - py[m - 1];
        const double bcx = px[m + 1] - px[m], bcy = py[m + 1] - py[m];
        const double acx = px[m + 1] - px[m - 1], acy = py[m + 1] - py[m - 1];
        const double cross = abx * bcy - aby * bcx;
        const double lab = std::sqrt(abx * abx + aby * aby), lbc = std::sqrt(bcx * bcx + bcy * bcy),
                     lac = std::sqrt(acx * acx + acy * acy);
        const double kappa = (lab == 0.0 || lbc == 0.0 || lac == 0.0) ? 0.0 : 2.0 * cross / (lab * lbc * lac);
        out.curvature[valid[m]] = kappa;
        if (kappa > best) {  // strictly: ties stay with the smaller index
            best = kappa;
            out.selected = valid[m];
            out.found = 1;
        }
    }
    if (!out.found && !valid.empty()) {  // the fallback if valid, else the valid index nearest to it (ties: smaller)
        int pick = valid[0];
        for (int i : valid)
            if (std::abs(i - fallback) < std::abs(pick - fallback)) pick = i;
        out.selected = pick;
    }
    return out;
}

#ifdef SART_HAVE_HDF5

namespace {

void create_scan(hid_t grp, const char* name, hid_t ftype, const std::vector<hsize_t>& dims, bool chunk_rows) {
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
    if (!ds.valid()) throw Error(std::string("Unable to create dataset beta_scan/") + name + ".");
}

}  // namespace

ScanWriter::ScanWriter(const std::string& filename, uint64_t frames, uint64_t nb, uint64_t nvoxel, const double* beta)
    : filename_(filename), frames_(frames), nb_(nb), nvox_(nvoxel) {
    if (nvox_ == 0) throw Error("Argument nvoxel must be positive.");
    if (nb_ == 0) throw Error("A beta scan needs at least one weight.");
    SART_H5_LOCK;
    file_ = h5_create_file(filename_);
    H5Id g = h5_create_group(file_, "beta_scan");
    h5_write_f64(g, "beta", {nb_}, beta);
    create_scan(g, "value", H5T_IEEE_F64LE, {frames_, nb_, nvox_}, true);
    create_scan(g, "status", H5T_STD_I32LE, {frames_, nb_}, false);
    create_scan(g, "iterations", H5T_STD_I32LE, {frames_, nb_}, false);
    create_scan(g, "residual_norm", H5T_IEEE_F64LE, {frames_, nb_}, false);
    create_scan(g, "roughness_norm", H5T_IEEE_F64LE, {frames_, nb_}, false);
    create_scan(g, "curvature", H5T_IEEE_F64LE, {frames_, nb_}, false);
    create_scan(g, "selected", H5T_STD_I32LE, {frames_}, false);
    create_scan(g, "corner_found", H5T_STD_U8LE, {frames_}, false);
}

hid_t ScanWriter::file() {
    if (!file_.valid()) file_ = h5_open_file(filename_, true);
    return file_;
}

void ScanWriter::close() {
    SART_H5_LOCK;
    file_.reset();
}

void ScanWriter::write_column(uint64_t k, uint64_t i, const double* x, int32_t status, int32_t iterations) {
    if (k >= frames_ || i >= nb_) throw Error("Beta scan column " + std::to_string(k) + ", " + std::to_string(i) + " is out of bounds.");
    SART_H5_LOCK;
    const hid_t f = file();
    {
        H5Id ds = h5_open_dataset(f, "beta_scan/value");
        h5_write_box(ds, {k, i, 0}, {1, 1, nvox_}, H5T_NATIVE_DOUBLE, x);
    }
    {
        H5Id ds = h5_open_dataset(f, "beta_scan/status");
        h5_write_box(ds, {k, i}, {1, 1}, H5T_NATIVE_INT32, &status);
    }
    H5Id ds = h5_open_dataset(f, "beta_scan/iterations");
    h5_write_box(ds, {k, i}, {1, 1}, H5T_NATIVE_INT32, &iterations);
}

void ScanWriter::read_columns(uint64_t j0, uint64_t n, double* out) {
    if (j0 + n > frames_ * nb_) throw Error("Beta scan rows beyond the stored columns.");
    SART_H5_LOCK;
    H5Id ds = h5_open_dataset(file(), "beta_scan/value");
    H5Id fsp(H5Dget_space(ds), H5Id::kSpace);
    hsize_t m = nvox_;
    H5Id msp(H5Screate_simple(1, &m, nullptr), H5Id::kSpace);
    for (uint64_t j = j0; j < j0 + n; ++j) {  // a group may straddle two composite frames: one column at a time
        hsize_t o[3] = {j / nb_, j % nb_, 0}, c[3] = {1, 1, nvox_};
        H5Sselect_hyperslab(fsp, H5S_SELECT_SET, o, nullptr, c, nullptr);
        if (H5Dread(ds, H5T_NATIVE_DOUBLE, msp, fsp, H5P_DEFAULT, out + (j - j0) * nvox_) < 0)
            throw Error("Unable to read beta_scan/value of " + filename_ + ".");
    }
}

void ScanWriter::write_frame(uint64_t k, const double* rho, const double* eta, const double* curvature,
                             int32_t selected, uint8_t found) {
    if (k >= frames_) throw Error("Beta scan frame " + std::to_string(k) + " is out of bounds.");
    SART_H5_LOCK;
    const hid_t f = file();
    auto put = [&](const char* name, const std::vector<uint64_t>& off, const std::vector<uint64_t>& cnt, hid_t mtype,
                   const void* data) {
        H5Id ds = h5_open_dataset(f, std::string("beta_scan/") + name);
        h5_write_box(ds, off, cnt, mtype, data);
    };
    put("residual_norm", {k, 0}, {1, nb_}, H5T_NATIVE_DOUBLE, rho);
    put("roughness_norm", {k, 0}, {1, nb_}, H5T_NATIVE_DOUBLE, eta);
    put("curvature", {k, 0}, {1, nb_}, H5T_NATIVE_DOUBLE, curvature);
    put("selected", {k}, {1}, H5T_NATIVE_INT32, &selected);
    put("corner_found", {k}, {1}, H5T_NATIVE_UINT8, &found);
}

#endif  // SART_HAVE_HDF5

}  // namespace sart
