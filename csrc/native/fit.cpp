#include "fit.hpp"

#include <cmath>
#include <stdexcept>

namespace sart {

void cpu_fit_forward(const float* A, int64_t P, int64_t V, int64_t ld, const double* X, int64_t ldx, int nv, double* F,
                     int64_t ldf) {
    if (nv < 0 || P < 0 || V < 0 || ld < V || ldx < V || ldf < P)
        throw std::invalid_argument("cpu_fit_forward: bad shape");
#pragma omp parallel for schedule(static)
    for (int64_t p = 0; p < P; ++p) {
        const float* row = A + p * ld;
        for (int j = 0; j < nv; ++j) {
            const double* x = X + (int64_t)j * ldx;
            double s = 0.0;
            for (int64_t v = 0; v < V; ++v) s += (double)row[v] * x[v];
            F[(int64_t)j * ldf + p] = s;
        }
    }
}

void cpu_fit_forward(const HostCsr& rows, const double* X, int64_t ldx, int nv, double* F, int64_t ldf) {
    csr_validate(rows, "cpu_fit_forward");
    if (nv < 0 || ldx < rows.ncols || ldf < rows.nrows) throw std::invalid_argument("cpu_fit_forward: bad shape");
#pragma omp parallel for schedule(static)
    for (int64_t p = 0; p < rows.nrows; ++p) {
        const int64_t k0 = rows.ptr[p], k1 = rows.ptr[p + 1];
        for (int j = 0; j < nv; ++j) {
            const double* x = X + (int64_t)j * ldx;
            double s = 0.0;
            for (int64_t k = k0; k < k1; ++k) s += (double)rows.val[k] * x[rows.idx[k]];
            F[(int64_t)j * ldf + p] = s;
        }
    }
}

FitStats fit_statistics(const double* f, const double* g, const double* ell, int64_t npixel, double threshold,
                        const std::vector<int64_t>& camera_pixels) {
    int64_t total = 0;
    for (int64_t n : camera_pixels) {
        if (n < 0) throw std::invalid_argument("fit_statistics: negative camera pixel count");
        total += n;
    }
    if (npixel < 0 || total != npixel)
        throw std::invalid_argument("fit_statistics: the cameras' pixel counts must sum to npixel");
    FitStats s;
    const size_t ncam = camera_pixels.size();
    s.residual_norm_camera.assign(ncam, 0.0);
    s.measurement_norm_camera.assign(ncam, 0.0);
    s.pixels_camera.assign(ncam, 0);
    double r2 = 0.0, g2 = 0.0;
    int64_t p = 0;
    for (size_t c = 0; c < ncam; ++c) {
        double cr2 = 0.0, cg2 = 0.0;
        int64_t cn = 0;
        for (const int64_t end = p + camera_pixels[c]; p < end; ++p) {
            if (!(g[p] >= 0.0) || !(ell[p] > threshold)) continue;  // saturated (or NaN) pixel, or no ray length
            const double r = g[p] - f[p];
            const double a = std::fabs(r);
            cr2 += r * r;
            cg2 += g[p] * g[p];
            r2 += r * r;
            g2 += g[p] * g[p];
            // a non-finite residual stays visible in the maximum (max(x, NaN) would drop it)
            if (a > s.residual_max || a != a) s.residual_max = a;
            ++cn;
        }
        s.residual_norm_camera[c] = std::sqrt(cr2);
        s.measurement_norm_camera[c] = std::sqrt(cg2);
        s.pixels_camera[c] = cn;
        s.pixels += cn;
    }
    s.residual_norm = std::sqrt(r2);
    s.measurement_norm = std::sqrt(g2);
    return s;
}

#ifdef SART_HAVE_HDF5

namespace {

void create_rows(hid_t grp, const char* name, hid_t ftype, uint64_t rows, uint64_t cols) {
    // [rows] or [rows][cols]; the image in chunks of one row
    hsize_t dims[2] = {rows, cols};
    const int rank = cols ? 2 : 1;
    H5Id sp(H5Screate_simple(rank, dims, nullptr), H5Id::kSpace);
    H5Id pl(H5Pcreate(H5P_DATASET_CREATE), H5Id::kPlist);
    if (rank == 2 && rows > 0 && cols > 0) {
        hsize_t ch[2] = {1, cols};
        H5Pset_chunk(pl, 2, ch);
    }
    H5Id ds(H5Dcreate2(grp, name, ftype, sp, H5P_DEFAULT, pl, H5P_DEFAULT), H5Id::kDataset);
    if (!ds.valid()) throw Error(std::string("Unable to create dataset fit/") + name + ".");
}

}  // namespace

FitWriter::FitWriter(const std::string& filename, uint64_t frames, uint64_t npixel, uint64_t ncamera)
    : filename_(filename), frames_(frames), npix_(npixel), ncam_(ncamera) {
    if (npix_ == 0) throw Error("Argument npixel must be positive.");
    if (ncam_ == 0) throw Error("At least one camera is required.");
    SART_H5_LOCK;
    H5Id f = h5_open_file(filename_, true);
    if (h5_exists(f, "fit") && H5Ldelete(f, "fit", H5P_DEFAULT) < 0)
        throw Error("Unable to remove the fit group of " + filename_ + ".");
    H5Id g = h5_create_group(f, "fit");
    create_rows(g, "image", H5T_IEEE_F64LE, frames_, npix_);
    create_rows(g, "residual_norm", H5T_IEEE_F64LE, frames_, 0);
    create_rows(g, "measurement_norm", H5T_IEEE_F64LE, frames_, 0);
    create_rows(g, "residual_max", H5T_IEEE_F64LE, frames_, 0);
    create_rows(g, "pixels", H5T_STD_I64LE, frames_, 0);
    create_rows(g, "residual_norm_camera", H5T_IEEE_F64LE, frames_, ncam_);
    create_rows(g, "measurement_norm_camera", H5T_IEEE_F64LE, frames_, ncam_);
    create_rows(g, "pixels_camera", H5T_STD_I64LE, frames_, ncam_);
}

void FitWriter::write(uint64_t k, const double* image, const FitStats& s) {
    if (k >= frames_)
        throw Error("Fit row " + std::to_string(k) + " is out of bounds (" + std::to_string(frames_) + ").");
    if (s.residual_norm_camera.size() != ncam_ || s.measurement_norm_camera.size() != ncam_ ||
        s.pixels_camera.size() != ncam_)
        throw Error("One set of fit statistics per camera is required.");
    SART_H5_LOCK;
    H5Id f = h5_open_file(filename_, true);
    auto put = [&](const char* name, const std::vector<uint64_t>& off, const std::vector<uint64_t>& cnt, hid_t mtype,
                   const void* data) {
        H5Id ds = h5_open_dataset(f, std::string("fit/") + name);
        h5_write_box(ds, off, cnt, mtype, data);
    };
    const int64_t pixels = s.pixels;
    put("image", {k, 0}, {1, npix_}, H5T_NATIVE_DOUBLE, image);
    put("residual_norm", {k}, {1}, H5T_NATIVE_DOUBLE, &s.residual_norm);
    put("measurement_norm", {k}, {1}, H5T_NATIVE_DOUBLE, &s.measurement_norm);
    put("residual_max", {k}, {1}, H5T_NATIVE_DOUBLE, &s.residual_max);
    put("pixels", {k}, {1}, H5T_NATIVE_INT64, &pixels);
    put("residual_norm_camera", {k, 0}, {1, ncam_}, H5T_NATIVE_DOUBLE, s.residual_norm_camera.data());
    put("measurement_norm_camera", {k, 0}, {1, ncam_}, H5T_NATIVE_DOUBLE, s.measurement_norm_camera.data());
    put("pixels_camera", {k, 0}, {1, ncam_}, H5T_NATIVE_INT64, s.pixels_camera.data());
}

std::vector<double> read_solution_times(const std::string& filename) {
    SART_H5_LOCK;
    h5_quiet();
    if (H5Fis_hdf5(filename.c_str()) <= 0) return {};
    H5Id f = h5_open_file(filename);
    if (!h5_exists(f, "solution/time") || !h5_exists(f, "solution/value")) return {};
    return h5_read_f64(f, "solution/time");
}

std::vector<double> read_solution_rows(const std::string& filename, uint64_t k0, uint64_t n, uint64_t nvoxel) {
    SART_H5_LOCK;
    H5Id f = h5_open_file(filename);
    H5Id ds = h5_open_dataset(f, "solution/value");
    const auto dims = h5_dims(ds);
    if (dims.size() != 2 || dims[1] != nvoxel)
        throw Error("solution/value of " + filename + " does not hold " + std::to_string(nvoxel) +
                    " voxels per frame.");
    if (k0 + n > dims[0]) throw Error("solution/value of " + filename + " holds fewer frames than solution/time.");
    std::vector<double> out(n * nvoxel);
    if (n == 0) return out;
    H5Id fsp(H5Dget_space(ds), H5Id::kSpace);
    hsize_t o[2] = {k0, 0}, c[2] = {n, nvoxel};
    H5Sselect_hyperslab(fsp, H5S_SELECT_SET, o, nullptr, c, nullptr);
    H5Id msp(H5Screate_simple(2, c, nullptr), H5Id::kSpace);
    if (H5Dread(ds, H5T_NATIVE_DOUBLE, msp, fsp, H5P_DEFAULT, out.data()) < 0)
        throw Error("Unable to read solution/value of " + filename + ".");
    return out;
}

#endif  // SART_HAVE_HDF5

}  // namespace sart
