#include "uncertainty.hpp"

#include <vector>

namespace sart {

#ifdef SART_HAVE_HDF5

namespace {

void create_sized(hid_t grp, const char* name, hid_t ftype, const std::vector<hsize_t>& dims, bool chunk_rows) {
    H5Id sp(H5Screate_simple((int)dims.size(), dims.data(), nullptr), H5Id::kSpace);
    H5Id pl(H5Pcreate(H5P_DATASET_CREATE), H5Id::kPlist);
    bool empty = false;
    for (hsize_t d : dims) empty = empty || d == 0;
    if (chunk_rows && !empty) {  // one solution per chunk
        std::vector<hsize_t> ch(dims.size(), 1);
        ch.back() = dims.back();
        H5Pset_chunk(pl, (int)ch.size(), ch.data());
    }
    H5Id ds(H5Dcreate2(grp, name, ftype, sp, H5P_DEFAULT, pl, H5P_DEFAULT), H5Id::kDataset);
    if (!ds.valid()) throw Error(std::string("Unable to create dataset uncertainty/") + name + ".");
}

}  // namespace

UncertaintyWriter::UncertaintyWriter(const std::string& filename, uint64_t frames, uint64_t nrep, uint64_t nvoxel,
                                     const double noise[3], uint64_t seed, bool keep)
    : filename_(filename), frames_(frames), nrep_(nrep), nvox_(nvoxel), keep_(keep) {
    if (nvox_ == 0) throw Error("Argument nvoxel must be positive.");
    if (nrep_ < 2) throw Error("An uncertainty estimate needs at least two replicas.");
    SART_H5_LOCK;
    H5Id f = h5_create_file(filename_);
    H5Id g = h5_create_group(f, "uncertainty");
    h5_write_f64(g, "noise", {3}, noise);
    h5_write_u64(g, "seed", {1}, &seed);
    create_sized(g, "mean", H5T_IEEE_F64LE, {frames_, nvox_}, true);
    create_sized(g, "std", H5T_IEEE_F64LE, {frames_, nvox_}, true);
    create_sized(g, "count", H5T_STD_I32LE, {frames_}, false);
    create_sized(g, "status", H5T_STD_I32LE, {frames_, nrep_ + 1}, false);
    create_sized(g, "iterations", H5T_STD_I32LE, {frames_, nrep_ + 1}, false);
    if (keep_) create_sized(g, "value", H5T_IEEE_F64LE, {frames_, nrep_ + 1, nvox_}, true);
}

void UncertaintyWriter::write_frame(uint64_t k, const double* mean, const double* std_dev, int32_t count,
                                    const int32_t* status, const int32_t* iterations, const double* columns) {
    if (k >= frames_) throw Error("Uncertainty frame " + std::to_string(k) + " is out of bounds.");
    if (keep_ && !columns) throw Error("Uncertainty frame " + std::to_string(k) + " comes without its columns.");
    SART_H5_LOCK;
    H5Id f = h5_open_file(filename_, true);
    auto put = [&](const char* name, const std::vector<uint64_t>& off, const std::vector<uint64_t>& cnt, hid_t mtype,
                   const void* data) {
        H5Id ds = h5_open_dataset(f, std::string("uncertainty/") + name);
        h5_write_box(ds, off, cnt, mtype, data);
    };
    put("mean", {k, 0}, {1, nvox_}, H5T_NATIVE_DOUBLE, mean);
    put("std", {k, 0}, {1, nvox_}, H5T_NATIVE_DOUBLE, std_dev);
    put("count", {k}, {1}, H5T_NATIVE_INT32, &count);
    put("status", {k, 0}, {1, nrep_ + 1}, H5T_NATIVE_INT32, status);
    put("iterations", {k, 0}, {1, nrep_ + 1}, H5T_NATIVE_INT32, iterations);
    if (keep_) put("value", {k, 0, 0}, {1, nrep_ + 1, nvox_}, H5T_NATIVE_DOUBLE, columns);
}

#endif  // SART_HAVE_HDF5

}  // namespace sart
