// Python bindings of the gfx950 SART kernels (module mpi_cuda_sartsolver_amd._lib._sart_hip).
//
// The interface is deliberately ABI-neutral: device pointers and HIP streams are passed as integers
// (torch.Tensor.data_ptr(), torch.cuda.Stream.cuda_stream), so this module links only against the
// HIP runtime and works with any PyTorch-ROCm build. Launch functions never allocate, copy or
// synchronise, so callers may capture them into HIP graphs.
#include <hip/hip_runtime.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../engine/comm.hpp"
#include "../engine/engine.hpp"
#include "../engine/engine64.hpp"
#include "../engine/geometry.hpp"
#include "../engine/multiframe.hpp"
#include "../kernels/launchers.hpp"

namespace py = pybind11;


template <typename T>
static T* P(uintptr_t p) {
    return reinterpret_cast<T*>(p);
}
static hipStream_t S(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

using f64arr = py::array_t<double, py::array::c_style | py::array::forcecast>;

static py::dict solve_info(const sart::SolveInfo& i) {
    py::dict d;
    d["status"] = i.status;
    d["iterations"] = i.iterations;
    d["convergence"] = i.convergence;
    d["used_fused"] = i.used_fused;
    d["fused_variant"] = i.fused_variant;
    d["fallbacks"] = i.fallbacks;
    d["comm_fallbacks"] = i.comm_fallbacks;
    d["comm"] = std::string(i.comm ? i.comm : "");
    d["nonfinite"] = i.nonfinite;
    d["ms"] = i.ms;
    d["sweeps"] = i.sweeps;
    d["comm_ms"] = i.comm_ms;
    d["warm_from"] = i.warm_from;
    d["warm_iter"] = i.warm_iter;
    d["warm_live"] = i.warm_live;
    return d;
}

// The multi-frame plans as dicts (mf_plan_forward / mf_plan_backproject / mf_engine_plan, MultiFrameEngine.plan)
static py::dict mf_key_dict(const sart::MfKey& k) {
    py::dict d;
    d["path"] = sart::mf_path_name(k.path);
    d["forward"] = k.forward;
    d["ng"] = k.ng;
    d["depth"] = k.depth;
    d["tile"] = k.tile;
    d["kb"] = k.kb;
    d["lds"] = k.lds;
    d["as"] = k.as;
    d["early"] = k.early;
    d["nt"] = k.nt;
    d["mw"] = k.mw;
    return d;
}

static py::dict mf_fwd_plan_dict(const sart::MfFwdPlan& p) {
    py::dict d = mf_key_dict(p.key);
    d["nsplit"] = p.nsplit;
    d["cps"] = p.cps;
    d["grid"] = py::make_tuple(p.grid_x, p.nsplit);
    return d;
}

static py::dict mf_bwd_plan_dict(const sart::MfBwdPlan& p) {
    py::dict d = mf_key_dict(p.key);
    d["nsplit"] = p.nsplit;
    d["rps"] = p.rps;
    d["vox_align"] = p.vox_align;
    d["grid"] = py::make_tuple(p.grid_x(0, p.ld), p.nsplit);
    return d;
}

static py::dict mf_engine_plan_dict(const sart::MfEnginePlan& p) {
    py::dict d;
    d["storage"] = sart::rtm_storage_name(p.storage);
    d["sparse"] = p.sparse;
    d["nf"] = p.nf;
    d["split_a"] = p.split_a;
    d["fwd"] = p.sparse ? py::object(py::none()) : py::object(py::str(sart::mf_path_name(p.fwd)));
    d["bwd"] = p.sparse ? py::object(py::none()) : py::object(py::str(sart::mf_path_name(p.bwd)));
    d["forward_split"] = p.forward_split();
    d["backproject_split"] = p.backproject_split();
    d["xblk"] = p.xblk;
    d["fplan"] = p.sparse ? py::object(py::none()) : py::object(mf_fwd_plan_dict(p.fplan));
    d["bplan"] = p.sparse ? py::object(py::none()) : py::object(mf_bwd_plan_dict(p.bplan));
    d["nsf"] = p.nsf;
    d["nsb"] = p.nsb;
    d["nwb"] = p.nwb;
    d["pw"] = p.pw;
    d["needs_w_planes"] = p.needs_w_planes;
    d["qcap"] = p.qcap;
    d["rcap"] = p.rcap;
    d["chunk"] = p.chunk;
    d["admit_cap"] = p.admit_cap;
    d["src_age"] = p.src_age;
    d["src_finished"] = p.src_finished;
    d["lead"] = p.lead;
    d["src_extrap"] = p.src_extrap;
    d["drift"] = p.drift;
    d["stage_window"] = p.stage_window;
    d["skip_last_bwd"] = p.skip_last_bwd;
    d["use_graph"] = p.use_graph;
    d["fault_nan"] = p.fault_nan;
    d["vox_align"] = p.vox_align;
    d["chunks"] = py::cast(p.chunks);
    d["collectives"] = py::cast(p.collectives);
    d["describe"] = p.describe();
    return d;
}

static void bind_engine(py::module_& m) {
    py::enum_<sart::ReduceOp>(m, "ReduceOp", py::module_local()).value("SUM", sart::ReduceOp::kSum).value("MAX", sart::ReduceOp::kMax);
    py::class_<sart::Communicator, std::shared_ptr<sart::Communicator>>(m, "Comm")
        .def_property_readonly("rank", [](sart::Communicator& c) { return c.rank(); })
        .def_property_readonly("size", [](sart::Communicator& c) { return c.size(); })
        .def_property_readonly("backend", &sart::Communicator::backend)
        .def_property_readonly("describe", &sart::Communicator::describe)
        .def_property_readonly("setup_seconds", &sart::Communicator::setup_seconds)
        .def("prepare", &sart::Communicator::prepare, py::arg("float_sizes"), py::call_guard<py::gil_scoped_release>())
        .def("check", &sart::Communicator::check)
        .def("device_failed", &sart::Communicator::device_failed)
        .def_property_readonly("degradable", &sart::Communicator::degradable)
        .def("degrade", &sart::Communicator::degrade)
        .def("barrier", [](sart::Communicator& c) { c.host().barrier(); }, py::call_guard<py::gil_scoped_release>())
        .def("abort", &sart::Communicator::abort)
        .def("all_reduce_host",
             [](sart::Communicator& c, f64arr v, sart::ReduceOp op) {
                 py::array_t<double> out(v.size());
                 std::memcpy(out.mutable_data(), v.data(), v.size() * sizeof(double));
                 double* p = out.mutable_data();
                 const size_t n = (size_t)v.size();
                 {
                     py::gil_scoped_release rel;
                     c.host().all_reduce_host(p, n, op);
                 }
                 return out;
             })
        .def("broadcast_bytes",
             [](sart::Communicator& c, py::bytes data, size_t nbytes, int root) {
                 std::string buf(nbytes, '\0');
                 if (c.rank() == root) {
                     const std::string d = data;
                     if (d.size() != nbytes) throw py::value_error("broadcast_bytes: root payload size mismatch");
                     buf = d;
                 }
                 {
                     py::gil_scoped_release rel;
                     c.host().broadcast_host(buf.data(), nbytes, root);
                 }
                 return py::bytes(buf);
             })
        .def("all_reduce_device",
             [](sart::Communicator& c, uintptr_t ptr, size_t n, bool f64, sart::ReduceOp op, uintptr_t stream) {
                 py::gil_scoped_release rel;
                 if (f64)
                     c.all_reduce(P<double>(ptr), n, op, S(stream));
                 else
                     c.all_reduce(P<float>(ptr), n, op, S(stream));
             });
    m.def("local_comm", []() { return std::shared_ptr<sart::Communicator>(sart::make_local_comm()); });
    m.def("staged_comm",
          [](int rank, int size, const std::string& host, int port, double timeout_s) {
              py::gil_scoped_release rel;
              return std::shared_ptr<sart::Communicator>(
                  sart::make_staged_comm(sart::make_tcp_host_comm(rank, size, host, port, timeout_s)));
          },
          py::arg("rank"), py::arg("size"), py::arg("host"), py::arg("port"), py::arg("timeout_s") = 3600.0);
    m.def("rccl_unique_id", []() { return py::bytes(sart::rccl_unique_id()); });
    m.def("rccl_comm",
          [](int device, py::bytes uid, int rank, int size, const std::string& host, int port) {
              const std::string id = uid;
              py::gil_scoped_release rel;
              return std::shared_ptr<sart::Communicator>(
                  sart::make_rccl_comm(device, id, sart::make_tcp_host_comm(rank, size, host, port)));
          });
    m.def("p2p_comm",
          [](int device, std::shared_ptr<sart::Communicator> base) {
              py::gil_scoped_release rel;
              return std::shared_ptr<sart::Communicator>(sart::make_p2p_comm(device, std::move(base)));
          },
          py::arg("device"), py::arg("base"));
    m.def("comm_from_env", [](int device) {
        py::gil_scoped_release rel;
        return std::shared_ptr<sart::Communicator>(sart::comm_from_env(device));
    });

    // (writable and constructible: the planner's tests hand fused_plan geometries fused_geometry never returns)
    py::class_<sart::FusedGeometry>(m, "FusedGeometry")
        .def(py::init<>())
        .def_readwrite("K", &sart::FusedGeometry::K)
        .def_readwrite("J", &sart::FusedGeometry::J)
        .def_readwrite("I", &sart::FusedGeometry::I)
        .def_readwrite("grid", &sart::FusedGeometry::grid)
        .def_readwrite("variant", &sart::FusedGeometry::variant)
        .def_readwrite("T", &sart::FusedGeometry::T)
        .def_readwrite("cpl", &sart::FusedGeometry::cpl)
        .def_readwrite("kw", &sart::FusedGeometry::kw)
        .def_readwrite("xl", &sart::FusedGeometry::xl)
        .def("valid", &sart::FusedGeometry::valid);
    m.def("fused_geometry", &sart::fused_geometry, py::arg("ld"), py::arg("num_cus"), py::arg("variant") = 6,
          py::arg("rows_per_tile") = 0, py::arg("narrow_slabs") = true, py::arg("chip_wide") = true);
    m.def("fused_geometry_bf16_wide", &sart::fused_geometry_bf16_wide, py::arg("ld"), py::arg("num_cus"));
    m.def("fused_fold_tiles", &sart::fused_fold_tiles, py::arg("geometry"), py::arg("nrows_pad"));
    m.def("fused_chain_plan", [](const sart::FusedGeometry& g, int64_t nrows_pad, bool split) {
        const auto p = sart::fused_chain_plan(g, nrows_pad, split);
        return py::make_tuple(p.chain_tiles, p.blocks);
    }, py::arg("geometry"), py::arg("nrows_pad"), py::arg("split_schedule"));
    auto fused_key_dict = [](const sart::FusedKey& k) {
        using namespace pybind11::literals;
        return py::dict("storage"_a = sart::rtm_storage_name(k.storage), "variant"_a = k.variant, "xl"_a = k.xl,
                        "diag"_a = k.diag, "T"_a = k.T, "sched"_a = k.sched, "cpl"_a = k.cpl, "kw"_a = k.kw);
    };
    // The launch plan of the fused sweep for a geometry and a storage ("f32", "bf16", "f16") under the knobs as they are
    // now. With ld > 0 also what a launch checks first (fused_check_launch: the shape, then that the kernel is built).
    m.def("fused_plan", [fused_key_dict](const sart::FusedGeometry& g, const std::string& storage, int64_t ld,
                                         int64_t nrows_pad, int64_t chain_tiles) {
        const sart::FusedPlan p = sart::fused_plan(g, sart::rtm_storage_from_name(storage.c_str()),
                                                   sart::FusedKnobs::current());
        if (ld > 0) sart::fused_check_launch(p, ld, nrows_pad, g.I, g.J, chain_tiles, true);
        py::dict d = fused_key_dict(p.key);
        d["built"] = sart::fused_variant_built(p.key);
        d["split"] = p.split;
        d["threads"] = p.threads;
        d["lds_bytes"] = p.lds_bytes;
        d["dbg"] = p.dbg;
        return d;
    }, py::arg("geometry"), py::arg("storage"), py::arg("ld") = 0, py::arg("nrows_pad") = 0, py::arg("chain_tiles") = 0);
    // the built kernels of one storage (each exists for both LOG values): the lists of csrc/engine/fused_variants.hpp
    m.def("fused_variants", [fused_key_dict](const std::string& storage) {
        py::list out;
        for (const sart::FusedKey& k : sart::fused_variants(sart::rtm_storage_from_name(storage.c_str())))
            out.append(fused_key_dict(k));
        return out;
    }, py::arg("storage"));
    m.def("choose_ld", &sart::choose_ld, py::arg("nvoxel"), py::arg("max_waste") = 0.10,
          py::arg("narrow_slabs") = true);

    py::class_<sart::EngineConfig>(m, "EngineConfig")
        .def(py::init<>())
        .def_readwrite("logarithmic", &sart::EngineConfig::logarithmic)
        .def_readwrite("ray_density_threshold", &sart::EngineConfig::ray_density_threshold)
        .def_readwrite("ray_length_threshold", &sart::EngineConfig::ray_length_threshold)
        .def_readwrite("conv_tolerance", &sart::EngineConfig::conv_tolerance)
        .def_readwrite("beta_laplace", &sart::EngineConfig::beta_laplace)
        .def_readwrite("relaxation", &sart::EngineConfig::relaxation)
        .def_readwrite("max_iterations", &sart::EngineConfig::max_iterations)
        .def_readwrite("allow_zero_tolerance", &sart::EngineConfig::allow_zero_tolerance)
        .def_readwrite("check_interval", &sart::EngineConfig::check_interval)
        .def_readwrite("use_fused", &sart::EngineConfig::use_fused)
        .def_readwrite("mf_frames", &sart::EngineConfig::mf_frames)
        .def_readwrite("mf_frame_beta", &sart::EngineConfig::mf_frame_beta)
        .def_readwrite("fused_min_bytes", &sart::EngineConfig::fused_min_bytes)
        .def_readwrite("column_shard", &sart::EngineConfig::column_shard)
        .def_readwrite("col_offset", &sart::EngineConfig::col_offset)
        .def_readwrite("nvoxel_total", &sart::EngineConfig::nvoxel_total)
        .def_readwrite("fused_variant", &sart::EngineConfig::fused_variant)
        .def_readwrite("rows_per_tile", &sart::EngineConfig::rows_per_tile)
        .def_readwrite("fused_schedule", &sart::EngineConfig::fused_schedule)
        .def_readwrite("use_graph", &sart::EngineConfig::use_graph)
        .def_readwrite("time_collectives", &sart::EngineConfig::time_collectives)
        .def_readwrite("rtm_bf16", &sart::EngineConfig::rtm_bf16)
        // row-scaled f16 storage: row_scale is the device pointer of the shard's scale array ([nrows_pad] scales,
        // then [nrows_pad] inverses; the caller keeps it alive with the engine)
        .def_readwrite("rtm_f16", &sart::EngineConfig::rtm_f16)
        .def_readwrite("f16_fused", &sart::EngineConfig::f16_fused)
        .def_property("row_scale",
                      [](const sart::EngineConfig& c) { return reinterpret_cast<uintptr_t>(c.row_scale); },
                      [](sart::EngineConfig& c, uintptr_t p) { c.row_scale = P<const float>(p); })
        .def_readwrite("mf_split_a", &sart::EngineConfig::mf_split_a)
        .def_readwrite("fault_inject", &sart::EngineConfig::fault_inject)
        .def_readwrite("fault_nan_sweep", &sart::EngineConfig::fault_nan_sweep)
        .def_readwrite("fused_max_cus", &sart::EngineConfig::fused_max_cus);
    m.def("validate_config", [](const sart::EngineConfig& c) {
        try {
            sart::validate_params(c);
        } catch (const std::invalid_argument& e) {
            throw py::value_error(e.what());
        }
    });

    py::class_<sart::Engine>(m, "Engine")
        .def(py::init([](int device, uintptr_t A, int64_t nrows, int64_t nrows_pad, int64_t nvoxel, int64_t ld,
                         std::shared_ptr<sart::Communicator> comm, const sart::EngineConfig& cfg) {
                 try {
                     return new sart::Engine(device, P<const float>(A), nrows, nrows_pad, nvoxel, ld, comm.get(), cfg);
                 } catch (const std::invalid_argument& e) {
                     throw py::value_error(e.what());
                 }
             }),
             py::keep_alive<1, 8>())
        // sparse shard: device pointers of the CSR (row_ptr, col, val) and CSC (col_ptr, row, cval) arrays (not owned:
        // the caller keeps them alive with the engine)
        .def_static("from_sparse",
                    [](int device, uintptr_t row_ptr, uintptr_t col, uintptr_t val, uintptr_t col_ptr, uintptr_t row,
                       uintptr_t cval, int64_t nnz, int64_t nrows, int64_t nvoxel,
                       std::shared_ptr<sart::Communicator> comm, const sart::EngineConfig& cfg) {
                        sart::SparseRtm s;
                        s.row_ptr = P<const int64_t>(row_ptr);
                        s.col = P<const int32_t>(col);
                        s.val = P<const float>(val);
                        s.col_ptr = P<const int64_t>(col_ptr);
                        s.row = P<const int32_t>(row);
                        s.cval = P<const float>(cval);
                        s.nnz = nnz;
                        const int64_t pp = (nrows + 63) / 64 * 64, ld = (nvoxel + 63) / 64 * 64;
                        try {
                            return new sart::Engine(device, nullptr, nrows, pp, nvoxel, ld, comm.get(), cfg, &s);
                        } catch (const std::invalid_argument& e) {
                            throw py::value_error(e.what());
                        }
                    },
                    py::keep_alive<0, 11>())
        .def("set_laplacian",
             [](sart::Engine& e, py::array_t<int64_t, py::array::c_style | py::array::forcecast> rp,
                py::array_t<int32_t, py::array::c_style | py::array::forcecast> col,
                py::array_t<float, py::array::c_style | py::array::forcecast> val) {
                 e.set_laplacian(rp.data(), col.data(), val.data(), (int64_t)val.size());
             })
        .def("solve",
             [](sart::Engine& e, f64arr g, py::object x0) {
                 if ((int64_t)g.size() != e.nrows())
                     throw py::value_error("measurement has " + std::to_string(g.size()) +
                                           " pixels, the local shard has " + std::to_string(e.nrows()));
                 f64arr x0a;
                 const double* x0p = nullptr;
                 if (!x0.is_none()) {
                     x0a = x0.cast<f64arr>();
                     if ((int64_t)x0a.size() != e.nvoxel())
                         throw py::value_error("Solution vector must be empty or contain nvoxel elements.");
                     x0p = x0a.data();
                 }
                 py::array_t<double> x(e.nvoxel());
                 double* xp = x.mutable_data();
                 const double* gp = g.data();
                 sart::SolveInfo info;
                 {
                     py::gil_scoped_release rel;
                     info = e.solve(gp, x0p, xp);
                 }
                 return py::make_tuple(x, solve_info(info));
             },
             py::arg("g"), py::arg("x0") = py::none())
        .def("forward",
             [](sart::Engine& e, f64arr x) {
                 if ((int64_t)x.size() != e.nvoxel()) throw py::value_error("x must have nvoxel elements");
                 py::array_t<double> f(e.nrows());
                 e.forward(x.data(), f.mutable_data());
                 return f;
             })
        .def_property_readonly("use_fused", &sart::Engine::use_fused)
        .def_property_readonly("geometry", &sart::Engine::geometry)
        .def_property_readonly("num_cus", &sart::Engine::num_cus)
        .def_property_readonly("column_shard", &sart::Engine::column_shard)
        .def_property_readonly("sparse", &sart::Engine::sparse)
        .def_property_readonly("nnz", &sart::Engine::nnz)
        .def_property_readonly("shared_device", &sart::Engine::shared_device)
        .def_property_readonly("ranks_per_device", &sart::Engine::ranks_per_device)
        .def_property_readonly("plan_cus", &sart::Engine::plan_cus)
        .def_property_readonly("nrows", &sart::Engine::nrows)
        .def_property_readonly("nvoxel", &sart::Engine::nvoxel)
        .def_property_readonly("stream", [](const sart::Engine& e) { return reinterpret_cast<uintptr_t>(e.stream()); })
        .def("ray_density", [](const sart::Engine& e) { auto v = e.ray_density(); return py::array_t<double>(v.size(), v.data()); })
        .def("ray_length", [](const sart::Engine& e) { auto v = e.ray_length(); return py::array_t<double>(v.size(), v.data()); })        ;

    // The double-precision engine (fp32 dense row shards; cfg's storage / partition flags and `sparse` describe the
    // shard offered, and anything else is refused). gpu_semantics as CpuSolver's flag
    py::class_<sart::Engine64>(m, "Engine64")
        .def(py::init([](int device, uintptr_t A, int64_t nrows, int64_t nrows_pad, int64_t nvoxel, int64_t ld,
                         std::shared_ptr<sart::Communicator> comm, const sart::EngineConfig& cfg, bool gpu_semantics,
                         bool sparse) {
                 try {
                     const sart::SparseRtm s{};
                     return new sart::Engine64(device, P<const float>(A), nrows, nrows_pad, nvoxel, ld, comm.get(), cfg,
                                               gpu_semantics, sparse ? &s : nullptr);
                 } catch (const std::invalid_argument& e) {
                     throw py::value_error(e.what());
                 }
             }),
             py::arg("device"), py::arg("A"), py::arg("nrows"), py::arg("nrows_pad"), py::arg("nvoxel"), py::arg("ld"),
             py::arg("comm"), py::arg("cfg"), py::arg("gpu_semantics") = true, py::arg("sparse") = false,
             py::keep_alive<1, 8>())
        .def("set_laplacian",
             [](sart::Engine64& e, py::array_t<int64_t, py::array::c_style | py::array::forcecast> rp,
                py::array_t<int32_t, py::array::c_style | py::array::forcecast> col,
                py::array_t<float, py::array::c_style | py::array::forcecast> val) {
                 e.set_laplacian(rp.data(), col.data(), val.data(), (int64_t)val.size());
             })
        .def("solve",
             [](sart::Engine64& e, f64arr g, py::object x0) {
                 if ((int64_t)g.size() != e.nrows())
                     throw py::value_error("measurement has " + std::to_string(g.size()) +
                                           " pixels, the local shard has " + std::to_string(e.nrows()));
                 f64arr x0a;
                 const double* x0p = nullptr;
                 if (!x0.is_none()) {
                     x0a = x0.cast<f64arr>();
                     if ((int64_t)x0a.size() != e.nvoxel())
                         throw py::value_error("Solution vector must be empty or contain nvoxel elements.");
                     x0p = x0a.data();
                 }
                 py::array_t<double> x(e.nvoxel());
                 double* xp = x.mutable_data();
                 const double* gp = g.data();
                 sart::SolveInfo info;
                 {
                     py::gil_scoped_release rel;
                     info = e.solve(gp, x0p, xp);
                 }
                 return py::make_tuple(x, solve_info(info));
             },
             py::arg("g"), py::arg("x0") = py::none())
        .def_property_readonly("gpu_semantics", &sart::Engine64::gpu_semantics)
        .def_property_readonly("num_cus", &sart::Engine64::num_cus)
        .def_property_readonly("nrows", &sart::Engine64::nrows)
        .def_property_readonly("nvoxel", &sart::Engine64::nvoxel)
        .def_property_readonly("stream", [](const sart::Engine64& e) { return reinterpret_cast<uintptr_t>(e.stream()); })
        .def("ray_density", [](const sart::Engine64& e) { auto v = e.ray_density(); return py::array_t<double>(v.size(), v.data()); })
        .def("ray_length", [](const sart::Engine64& e) { auto v = e.ray_length(); return py::array_t<double>(v.size(), v.data()); });

    py::class_<sart::MultiFrameEngine>(m, "MultiFrameEngine")
        .def(py::init([](int device, uintptr_t A, int64_t nrows, int64_t nrows_pad, int64_t nvoxel, int64_t ld,
                         std::shared_ptr<sart::Communicator> comm, const sart::EngineConfig& cfg) {
                 try {
                     return new sart::MultiFrameEngine(device, P<const void>(A), nrows, nrows_pad, nvoxel, ld,
                                                       comm.get(), cfg);
                 } catch (const std::invalid_argument& e) {
                     throw py::value_error(e.what());
                 }
             }),
             py::keep_alive<1, 8>())
        .def_static("from_sparse",
                    [](int device, uintptr_t row_ptr, uintptr_t col, uintptr_t val, uintptr_t col_ptr, uintptr_t row,
                       uintptr_t cval, int64_t nnz, int64_t nrows, int64_t nvoxel,
                       std::shared_ptr<sart::Communicator> comm, const sart::EngineConfig& cfg) {
                        sart::SparseRtm s;
                        s.row_ptr = P<const int64_t>(row_ptr);
                        s.col = P<const int32_t>(col);
                        s.val = P<const float>(val);
                        s.col_ptr = P<const int64_t>(col_ptr);
                        s.row = P<const int32_t>(row);
                        s.cval = P<const float>(cval);
                        s.nnz = nnz;
                        const int64_t pp = (nrows + 63) / 64 * 64, ld = (nvoxel + 63) / 64 * 64;
                        try {
                            return new sart::MultiFrameEngine(device, nullptr, nrows, pp, nvoxel, ld, comm.get(), cfg,
                                                              &s);
                        } catch (const std::invalid_argument& e) {
                            throw py::value_error(e.what());
                        }
                    },
                    py::keep_alive<0, 11>())
        .def_property_readonly("plan", [](const sart::MultiFrameEngine& e) { return mf_engine_plan_dict(e.plan()); })
        .def_property_readonly("sparse", &sart::MultiFrameEngine::sparse)
        .def_property_readonly("batch_frames", &sart::MultiFrameEngine::batch_frames)
        .def_property_readonly("split_a", &sart::MultiFrameEngine::split_a)
        .def_property_readonly("forward_split", &sart::MultiFrameEngine::forward_split)
        .def_property_readonly("backproject_split", &sart::MultiFrameEngine::backproject_split)
        .def("set_laplacian",
             [](sart::MultiFrameEngine& e, py::array_t<int64_t, py::array::c_style | py::array::forcecast> rp,
                py::array_t<int32_t, py::array::c_style | py::array::forcecast> col,
                py::array_t<float, py::array::c_style | py::array::forcecast> val) {
                 e.set_laplacian(rp.data(), col.data(), val.data(), (int64_t)val.size());
             })
        .def("solve_batch", [](sart::MultiFrameEngine& e, f64arr g, py::object x0, bool chain, bool record_starts,
                               py::object betas) -> py::tuple {
            if (g.ndim() != 2 || g.shape(1) != e.nrows())
                throw py::value_error("measurements must be [nframes, nrows of the local shard]");
            const int nf = (int)g.shape(0);
            f64arr x0a;
            const double* x0p = nullptr;
            if (!x0.is_none()) {
                x0a = x0.cast<f64arr>();
                if ((int64_t)x0a.size() != e.nvoxel()) throw py::value_error("x0 must have nvoxel elements");
                x0p = x0a.data();
            }
            // betas (optional): a Laplacian weight per frame, nframes entries (fp32 on the device, as beta_laplace)
            py::array_t<float, py::array::c_style | py::array::forcecast> ba;
            const float* bp = nullptr;
            if (!betas.is_none()) {
                ba = betas.cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
                if ((int64_t)ba.size() != nf) throw py::value_error("betas must have one entry per frame");
                bp = ba.data();
            }
            py::array_t<double> x({(py::ssize_t)nf, (py::ssize_t)e.nvoxel()});
            py::array_t<double> st({(py::ssize_t)(record_starts ? nf : 0), (py::ssize_t)e.nvoxel()});
            double* xp = x.mutable_data();
            double* sp = record_starts ? st.mutable_data() : nullptr;
            const double* gp = g.data();
            std::vector<sart::SolveInfo> infos;
            try {
                py::gil_scoped_release rel;
                infos = e.solve_batch(gp, nf, xp, x0p, chain, sp, bp);
            } catch (const std::invalid_argument& ex) {
                throw py::value_error(ex.what());
            }
            py::list li;
            for (const auto& i : infos) li.append(solve_info(i));
            if (record_starts) return py::make_tuple(x, li, st);
            return py::make_tuple(x, li);
        }, py::arg("g"), py::arg("x0") = py::none(), py::arg("chain") = false, py::arg("record_starts") = false,
           py::arg("betas") = py::none())
        .def_property_readonly("series_stats", [](sart::MultiFrameEngine& e) {
            const auto& s = e.series_stats();
            py::dict d;
            d["frames"] = s.frames;
            d["sweeps"] = s.sweeps;
            d["queued_sweeps"] = s.queued_sweeps;
            d["busy_slot_sweeps"] = s.busy_slot_sweeps;
            d["chained"] = s.chained;
            d["slot_util"] = s.slot_util;
            d["mean_iterations"] = s.mean_iterations;
            d["mean_warm_age"] = s.mean_warm_age;
            d["ms"] = s.ms;
            d["chunk"] = s.chunk;
            d["admit_cap"] = s.admit_cap;
            d["src_age"] = s.src_age;
            d["restarts"] = s.restarts;
            d["src_finished"] = s.src_finished;
            d["lead"] = s.lead;
            d["src_extrap"] = s.src_extrap;
            d["drift"] = s.drift;
            d["stage_window"] = s.stage_window;
            d["host_wait_ms"] = s.host_wait_ms;
            d["host_stage_ms"] = s.host_stage_ms;
            d["host_src_ms"] = s.host_src_ms;
            d["host_deliver_ms"] = s.host_deliver_ms;
            return d;
        });
}

// Struct layouts for the tests (tests/mf_refill_model.py decodes raw device bytes of MfState / MfQueue with these, so
// python keeps no second copy of the structs): {"nbytes", "fields": {name: (offset, numpy dtype string, count)}}
#define MF_FIELD(S, name, dtype) \
    fields[#name] = py::make_tuple((int)offsetof(S, name), dtype, (int)(sizeof(S::name) / mf_dtype_size(dtype)))

static size_t mf_dtype_size(const char* dtype) { return (size_t)(dtype[2] - '0'); }

static py::dict mf_state_layout() {
    using S = sart::MfState;
    py::dict fields;
    MF_FIELD(S, G, "<f8");
    MF_FIELD(S, conv_prev, "<f8");
    MF_FIELD(S, conv, "<f8");
    MF_FIELD(S, done, "<i4");
    MF_FIELD(S, status, "<i4");
    MF_FIELD(S, iters, "<i4");
    MF_FIELD(S, sweep, "<i4");
    MF_FIELD(S, max_iter, "<i4");
    MF_FIELD(S, all_done, "<i4");
    MF_FIELD(S, nf, "<i4");
    MF_FIELD(S, flags, "<u8");
    MF_FIELD(S, tol, "<f8");
    MF_FIELD(S, rollback, "<u8");
    MF_FIELD(S, sweep0, "<i4");
    py::dict d;
    d["nbytes"] = (int)sizeof(S);
    d["fields"] = fields;
    return d;
}

static py::dict mf_finish_layout() {
    using S = sart::MfFinish;
    py::dict fields;
    MF_FIELD(S, frame, "<i4");
    MF_FIELD(S, status, "<i4");
    MF_FIELD(S, iters, "<i4");
    MF_FIELD(S, flags, "<i4");
    MF_FIELD(S, warm_from, "<i4");
    MF_FIELD(S, warm_iter, "<i4");
    MF_FIELD(S, warm_live, "<i4");
    MF_FIELD(S, conv, "<f8");
    MF_FIELD(S, norm, "<f8");
    py::dict d;
    d["nbytes"] = (int)sizeof(S);
    d["fields"] = fields;
    return d;
}

static py::dict mf_queue_layout() {
    using S = sart::MfQueue;
    py::dict fields;
    MF_FIELD(S, q_head, "<i8");
    MF_FIELD(S, q_tail, "<i8");
    MF_FIELD(S, fin, "<i8");
    MF_FIELD(S, drained, "<i8");
    MF_FIELD(S, qcap, "<i4");
    MF_FIELD(S, rcap, "<i4");
    MF_FIELD(S, chain, "<i4");
    MF_FIELD(S, admit_cap, "<i4");
    MF_FIELD(S, src_age, "<i4");
    MF_FIELD(S, src_finished, "<i4");
    MF_FIELD(S, lead, "<i4");
    MF_FIELD(S, src_extrap, "<f4");
    MF_FIELD(S, src_live, "<i4");
    MF_FIELD(S, x0_below, "<i8");
    MF_FIELD(S, n_ret, "<i4");
    MF_FIELD(S, n_adm, "<i4");
    MF_FIELD(S, upd_any, "<i4");
    MF_FIELD(S, skip_bwd, "<i4");
    MF_FIELD(S, xlast_frame, "<i4");
    MF_FIELD(S, xlast_iter, "<i4");
    MF_FIELD(S, xlast_slot, "<i4");
    MF_FIELD(S, xlast_norm, "<f8");
    MF_FIELD(S, xlast2_frame, "<i4");
    MF_FIELD(S, drift_frame1, "<i4");
    MF_FIELD(S, drift_frame2, "<i4");
    MF_FIELD(S, xlast2_norm, "<f8");
    MF_FIELD(S, drift_norm1, "<f8");
    MF_FIELD(S, drift_norm2, "<f8");
    MF_FIELD(S, drift, "<f4");
    MF_FIELD(S, src_kind, "<i4");
    MF_FIELD(S, src_slot, "<i4");
    MF_FIELD(S, src_frame, "<i4");
    MF_FIELD(S, src_iter, "<i4");
    MF_FIELD(S, src_norm, "<f8");
    MF_FIELD(S, slot_frame, "<i4");
    MF_FIELD(S, slot_warm_from, "<i4");
    MF_FIELD(S, slot_warm_iter, "<i4");
    MF_FIELD(S, slot_warm_live, "<i4");
    MF_FIELD(S, slot_norm, "<f8");
    MF_FIELD(S, ret_pos, "<i4");
    MF_FIELD(S, ret_prev, "<i4");
    MF_FIELD(S, adm_pos, "<i4");
    MF_FIELD(S, adm_kind, "<i4");
    MF_FIELD(S, q_frame, "<i4");
    MF_FIELD(S, q_cold, "<i4");
    MF_FIELD(S, q_norm, "<f8");
    MF_FIELD(S, q_G, "<f8");
    py::dict log = mf_finish_layout();  // MfFinish log[kMfQueueMax]: a sub-layout at its offset
    log["offset"] = (int)offsetof(S, log);
    log["count"] = (int)(sizeof(S::log) / sizeof(sart::MfFinish));
    py::dict d;
    d["nbytes"] = (int)sizeof(S);
    d["fields"] = fields;
    d["log"] = log;
    py::dict src;  // MfSrc
    src["none"] = (int)sart::kSrcNone, src["slot"] = (int)sart::kSrcSlot, src["last"] = (int)sart::kSrcLast;
    src["host_x0"] = (int)sart::kSrcHostX0, src["cold"] = (int)sart::kSrcCold;
    d["src"] = src;
    return d;
}
#undef MF_FIELD

// Test entry points of the multi-frame glue kernels (multiframe_glue.hip): thin wrappers over the launchers the
// engine calls, device pointers as integers (0: null)
static void bind_mf_glue(py::module_& m) {
    m.def("mf_state_layout", &mf_state_layout);
    m.def("mf_queue_layout", &mf_queue_layout);
    m.def("mf_max_frames", []() { return (int)sart::kMfMaxFrames; });
    m.def("mf_queue_max", []() { return (int)sart::kMfQueueMax; });
    m.def("mf_weights_num_blocks", &sart::mf_weights_num_blocks);
    m.def("lds_fill", [](unsigned word, uintptr_t sink, uintptr_t stream) {
        sart::launch_lds_fill(word, P<unsigned>(sink), S(stream));
    });
    m.def("mf_state_begin", [](uintptr_t st, uintptr_t G, int nused, double tol, int max_iter, int nf,
                               uintptr_t stream) {
        sart::launch_mf_state_begin(P<sart::MfState>(st), P<const double>(G), nused, tol, max_iter, nf, S(stream));
    }, py::arg("st"), py::arg("G"), py::arg("nused"), py::arg("tol"), py::arg("max_iter"), py::arg("nf"),
       py::arg("stream"));
    m.def("mf_queue_begin", [](uintptr_t q, int qcap, int rcap, bool chain, int admit_cap, int src_age,
                               int64_t x0_below, bool src_finished, bool lead, float src_extrap, float drift,
                               uintptr_t stream) {
        sart::launch_mf_queue_begin(P<sart::MfQueue>(q), qcap, rcap, chain, admit_cap, src_age, x0_below, src_finished,
                                    lead, src_extrap, S(stream), drift);
    }, py::arg("q"), py::arg("qcap"), py::arg("rcap"), py::arg("chain"), py::arg("admit_cap"), py::arg("src_age"),
       py::arg("x0_below"), py::arg("src_finished"), py::arg("lead"), py::arg("src_extrap"), py::arg("drift"),
       py::arg("stream"));
    m.def("mf_decide", [](uintptr_t st, uintptr_t F2, uintptr_t q, uintptr_t stream) {
        sart::launch_mf_decide(P<sart::MfState>(st), P<const float>(F2), S(stream), P<sart::MfQueue>(q));
    }, py::arg("st"), py::arg("F2"), py::arg("q"), py::arg("stream"));
    m.def("mf_update", [](uintptr_t X, uintptr_t D, uintptr_t O, uintptr_t pen, float alpha, bool logmode,
                          int64_t nvox, int64_t ld, uintptr_t st, int nf, uintptr_t Xprev, uintptr_t q,
                          uintptr_t ring, uintptr_t xlast, uintptr_t xlast2, uintptr_t x0, uintptr_t x0q, uintptr_t oq,
                          uintptr_t starts, uintptr_t stream) {
        sart::MfRefill rf{};
        rf.ring = P<float>(ring);
        rf.xlast = P<float>(xlast);
        rf.xlast2 = P<float>(xlast2);
        rf.x0 = P<const double>(x0);
        rf.x0q = P<const float>(x0q);
        rf.oq = P<const float>(oq);
        rf.starts = P<float>(starts);
        sart::launch_mf_update(P<float>(X), P<const float>(D), P<float>(O), P<const float>(pen), alpha, logmode, nvox,
                               ld, P<const sart::MfState>(st), nf, S(stream), P<float>(Xprev),
                               P<const sart::MfQueue>(q), q ? &rf : nullptr);
    }, py::arg("X"), py::arg("D"), py::arg("O"), py::arg("pen"), py::arg("alpha"), py::arg("logmode"),
       py::arg("nvox"), py::arg("ld"), py::arg("st"), py::arg("nf"), py::arg("Xprev"), py::arg("q"),
       py::arg("ring") = 0, py::arg("xlast") = 0, py::arg("xlast2") = 0, py::arg("x0") = 0, py::arg("x0q") = 0,
       py::arg("oq") = 0, py::arg("starts") = 0, py::arg("stream") = 0);
    m.def("mf_admit_rows", [](uintptr_t q, uintptr_t ghq, int64_t nrows, int64_t nrows_pad, uintptr_t ray_length,
                              float len_thres, uintptr_t ghat, uintptr_t arow, int nf, uintptr_t stream) {
        sart::launch_mf_admit_rows(P<const sart::MfQueue>(q), P<const float>(ghq), nrows, nrows_pad,
                                   P<const float>(ray_length), len_thres, P<float>(ghat), P<float>(arow), nf,
                                   S(stream));
    });
    m.def("mf_publish", [](uintptr_t q, int64_t q_tail, uintptr_t stream) {
        sart::launch_mf_publish(P<sart::MfQueue>(q), q_tail, S(stream));
    });
    m.def("mf_drained", [](uintptr_t q, int64_t drained, uintptr_t stream) {
        sart::launch_mf_drained(P<sart::MfQueue>(q), drained, S(stream));
    });
    m.def("mf_stage_stats", [](uintptr_t g64q, int64_t e0, int qcap, int k, int64_t nrows, int64_t nrows_pad,
                               uintptr_t stats, int nf, uintptr_t stream) {
        sart::launch_mf_stage_stats(P<const double>(g64q), e0, qcap, k, nrows, nrows_pad, P<double>(stats), nf,
                                    S(stream));
    });
    m.def("mf_stage_norm", [](uintptr_t q, uintptr_t g64q, uintptr_t ghq, uintptr_t stats, int64_t e0, int64_t frame0,
                              bool cold, int k, int64_t nrows, int64_t nrows_pad, int nf, uintptr_t stream) {
        sart::launch_mf_stage_norm(P<sart::MfQueue>(q), P<const double>(g64q), P<float>(ghq), P<const double>(stats),
                                   e0, frame0, cold, k, nrows, nrows_pad, nf, S(stream));
    });
    m.def("mf_stage_ops", [](uintptr_t ghq, int64_t e0, int qcap, int k, int64_t nrows, int64_t nrows_pad,
                             uintptr_t ray_length, float len_thres, uintptr_t gpos, uintptr_t wo, int nf,
                             uintptr_t stream) {
        sart::launch_mf_stage_ops(P<const float>(ghq), e0, qcap, k, nrows, nrows_pad, P<const float>(ray_length),
                                  len_thres, P<float>(gpos), P<float>(wo), nf, S(stream));
    });
    m.def("mf_stage_cols", [](uintptr_t D, uintptr_t dinv, int64_t e0, int qcap, int k, int64_t nvox, int64_t ld,
                              int nf, uintptr_t out, uintptr_t stream) {
        sart::launch_mf_stage_cols(P<const float>(D), P<const float>(dinv), e0, qcap, k, nvox, ld, nf, P<float>(out),
                                   S(stream));
    });
    m.def("mf_weights", [](uintptr_t Fs, int nsplit, int64_t nrows_pad, uintptr_t ghat, uintptr_t arow, bool logmode,
                           uintptr_t W, uintptr_t F2part, int nf, uintptr_t stream, uintptr_t wmax, int wplane) {
        sart::launch_mf_weights(P<const float>(Fs), nsplit, nrows_pad, P<const float>(ghat), P<const float>(arow),
                                logmode, P<float>(W), P<double>(F2part), nf, S(stream), P<unsigned>(wmax), wplane);
    }, py::arg("Fs"), py::arg("nsplit"), py::arg("nrows_pad"), py::arg("ghat"), py::arg("arow"), py::arg("logmode"),
       py::arg("W"), py::arg("F2part"), py::arg("nf"), py::arg("stream"), py::arg("wmax") = 0, py::arg("wplane") = 0);
    m.def("mf_collect", [](uintptr_t part, int nsplit, int64_t ld, int64_t v0, int64_t v1, uintptr_t scale,
                           uintptr_t D, uintptr_t F2part, int nF2, uintptr_t F2out, int nf, uintptr_t stream) {
        sart::launch_mf_collect(P<const float>(part), nsplit, ld, v0, v1, P<const float>(scale), P<float>(D),
                                P<const double>(F2part), nF2, P<float>(F2out), nf, S(stream));
    });
    m.def("mf_penalty", [](uintptr_t row_ptr, uintptr_t col, uintptr_t val, int64_t n, float beta, bool logx,
                           uintptr_t X, int64_t ld, uintptr_t pen, uintptr_t st, int nf, uintptr_t stream) {
        sart::launch_mf_penalty(P<const int64_t>(row_ptr), P<const int32_t>(col), P<const float>(val), n, beta, logx,
                                P<const float>(X), ld, P<float>(pen), P<const sart::MfState>(st), nf, S(stream));
    });
}

PYBIND11_MODULE(_sart_hip, m) {
    m.doc() = "Hand-written gfx950 (CDNA4) HIP kernels of the SART solver and the native engine";
    bind_engine(m);
    bind_mf_glue(m);

    m.def("arch", []() { return std::string("gfx950"); });
    m.def("state_nbytes", []() { return (int)sizeof(sart::SartState); });

    m.def("device_info", [](int dev) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) throw std::runtime_error("hipGetDeviceProperties failed");
        py::dict d;
        d["name"] = std::string(prop.name);
        d["gcnArchName"] = std::string(prop.gcnArchName);
        d["multiProcessorCount"] = prop.multiProcessorCount;
        d["totalGlobalMem"] = (int64_t)prop.totalGlobalMem;
        d["l2CacheSize"] = prop.l2CacheSize;
        d["clockRate_kHz"] = prop.clockRate;
        d["memoryClockRate_kHz"] = prop.memoryClockRate;
        d["memoryBusWidth"] = prop.memoryBusWidth;
        return d;
    });

    m.def("forward_num_blocks", &sart::forward_num_blocks);
    // bf16: A holds bf16 bit patterns (opt-in storage precision)
    m.def("forward", [](int epi, uintptr_t A, int64_t ld, int64_t nrows, int64_t nrows_pad, uintptr_t x,
                        uintptr_t ghat, uintptr_t arow, uintptr_t out_f, uintptr_t out_w, uintptr_t Fpart,
                        uintptr_t st, uintptr_t stream, bool bf16, bool f16, uintptr_t rinv) {
        if (f16 && bf16) throw std::runtime_error("forward: bf16 and f16 are exclusive");
        if (f16)  // row-scaled f16 bits; rinv: the rows' inverse scales
            sart::launch_forward(epi, P<const sart::f16s_t>(A), ld, nrows, nrows_pad, P<const float>(x),
                                 P<const float>(ghat), P<const float>(arow), P<float>(out_f), P<float>(out_w),
                                 P<double>(Fpart), P<const sart::SartState>(st), S(stream), P<const float>(rinv));
        else if (bf16)
            sart::launch_forward(epi, P<const sart::bf16_t>(A), ld, nrows, nrows_pad, P<const float>(x),
                                 P<const float>(ghat), P<const float>(arow), P<float>(out_f), P<float>(out_w),
                                 P<double>(Fpart), P<const sart::SartState>(st), S(stream));
        else
            sart::launch_forward(epi, P<const float>(A), ld, nrows, nrows_pad, P<const float>(x), P<const float>(ghat),
                                 P<const float>(arow), P<float>(out_f), P<float>(out_w), P<double>(Fpart),
                                 P<const sart::SartState>(st), S(stream));
    }, py::arg("epi"), py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("nrows_pad"), py::arg("x"),
       py::arg("ghat"), py::arg("arow"), py::arg("out_f"), py::arg("out_w"), py::arg("Fpart"), py::arg("st"),
       py::arg("stream"), py::arg("bf16") = false, py::arg("f16") = false, py::arg("rinv") = 0);
    m.def("rowsum_f64", [](uintptr_t A, int64_t ld, int64_t nrows, uintptr_t out, uintptr_t stream, bool bf16,
                           bool f16, uintptr_t rinv) {
        if (f16 && bf16) throw std::runtime_error("rowsum_f64: bf16 and f16 are exclusive");
        if (f16)
            sart::launch_rowsum_f64(P<const sart::f16s_t>(A), ld, nrows, P<double>(out), S(stream),
                                    P<const float>(rinv));
        else if (bf16)
            sart::launch_rowsum_f64(P<const sart::bf16_t>(A), ld, nrows, P<double>(out), S(stream));
        else
            sart::launch_rowsum_f64(P<const float>(A), ld, nrows, P<double>(out), S(stream));
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("out"), py::arg("stream"), py::arg("bf16") = false,
       py::arg("f16") = false, py::arg("rinv") = 0);
    m.def("backproject_num_splits", &sart::backproject_num_splits, py::arg("ld"), py::arg("nrows"),
          py::arg("elem_bytes") = 4);
    m.def("backproject", [](uintptr_t A, int64_t ld, int64_t nrows, uintptr_t w, int nsplit, uintptr_t partial,
                            uintptr_t st, uintptr_t stream, bool bf16, bool f16) {
        if (f16 && bf16) throw std::runtime_error("backproject: bf16 and f16 are exclusive");
        if (f16)  // w carries the rows' inverse scales
            sart::launch_backproject(P<const sart::f16s_t>(A), ld, nrows, P<const float>(w), nsplit,
                                     P<float>(partial), P<const sart::SartState>(st), S(stream));
        else if (bf16)
            sart::launch_backproject(P<const sart::bf16_t>(A), ld, nrows, P<const float>(w), nsplit,
                                     P<float>(partial), P<const sart::SartState>(st), S(stream));
        else
            sart::launch_backproject(P<const float>(A), ld, nrows, P<const float>(w), nsplit, P<float>(partial),
                                     P<const sart::SartState>(st), S(stream));
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("w"), py::arg("nsplit"), py::arg("partial"),
       py::arg("st"), py::arg("stream"), py::arg("bf16") = false, py::arg("f16") = false);
    m.def("colsum_f64", [](uintptr_t A, int64_t ld, int64_t nrows, int nsplit, uintptr_t partial, uintptr_t stream,
                           bool bf16, bool f16, uintptr_t rinv) {
        if (f16 && bf16) throw std::runtime_error("colsum_f64: bf16 and f16 are exclusive");
        if (f16)
            sart::launch_colsum_f64(P<const sart::f16s_t>(A), ld, nrows, nsplit, P<double>(partial), S(stream),
                                    P<const float>(rinv));
        else if (bf16)
            sart::launch_colsum_f64(P<const sart::bf16_t>(A), ld, nrows, nsplit, P<double>(partial), S(stream));
        else
            sart::launch_colsum_f64(P<const float>(A), ld, nrows, nsplit, P<double>(partial), S(stream));
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("nsplit"), py::arg("partial"), py::arg("stream"),
       py::arg("bf16") = false, py::arg("f16") = false, py::arg("rinv") = 0);
    // fp32 block of whole rows [n][ld] -> row-scaled f16 bits, scales and inverse scales (n each); flushed: optional
    // device counters (two uint64: the non-zero inputs stored as zero or subnormal, all non-zero inputs)
    m.def("f32_to_f16_rows", [](uintptr_t src, int64_t n, int64_t ld, int64_t nvoxel, uintptr_t dst, uintptr_t scale,
                                uintptr_t inv_scale, uintptr_t flushed, uintptr_t stream) {
        sart::launch_f32_to_f16_rows(P<const float>(src), n, ld, nvoxel, P<sart::f16s_t>(dst), P<float>(scale),
                                     P<float>(inv_scale), P<unsigned long long>(flushed), S(stream));
    }, py::arg("src"), py::arg("n"), py::arg("ld"), py::arg("nvoxel"), py::arg("dst"), py::arg("scale"),
       py::arg("inv_scale"), py::arg("flushed"), py::arg("stream"));
    m.def("scale_rows", [](uintptr_t v, uintptr_t rinv, int64_t n, uintptr_t stream) {
        sart::launch_scale_rows(P<float>(v), P<const float>(rinv), n, S(stream));
    });
    m.def("f32_to_bf16", [](uintptr_t src, int64_t n, uintptr_t dst, uintptr_t stream) {
        sart::launch_f32_to_bf16(P<const float>(src), n, P<sart::bf16_t>(dst), S(stream));
    });
    m.def("reduce_partials", [](uintptr_t partial, int64_t ld, int nsplit, uintptr_t scale, uintptr_t out,
                                uintptr_t Fpart, int64_t nF, uintptr_t Fout, uintptr_t st, uintptr_t stream) {
        sart::launch_reduce_partials(P<const float>(partial), ld, nsplit, P<const float>(scale), P<float>(out),
                                     P<const double>(Fpart), nF, P<float>(Fout), P<const sart::SartState>(st),
                                     S(stream));
    });
    m.def("reduce_partials_f64", [](uintptr_t partial, int64_t ld, int nsplit, uintptr_t out, uintptr_t stream) {
        sart::launch_reduce_partials_f64(P<const double>(partial), ld, nsplit, P<double>(out), S(stream));
    });
    // projection64.hip: the fp64 two-pass kernels (fp32 shard, fp64 vectors)
    m.def("forward64", [](int epi, uintptr_t A, int64_t ld, int64_t nrows, int64_t nrows_pad, int64_t nvoxel,
                          uintptr_t x, uintptr_t g, uintptr_t arow, uintptr_t out_f, uintptr_t out_w, uintptr_t Fpart,
                          uintptr_t st, uintptr_t stream) {
        sart::launch_forward64(epi, P<const float>(A), ld, nrows, nrows_pad, nvoxel, P<const double>(x),
                               P<const double>(g), P<const double>(arow), P<double>(out_f), P<double>(out_w),
                               P<double>(Fpart), P<const sart::SartState>(st), S(stream));
    }, py::arg("epi"), py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("nrows_pad"), py::arg("nvoxel"),
       py::arg("x"), py::arg("g"), py::arg("arow"), py::arg("out_f"), py::arg("out_w"), py::arg("Fpart"),
       py::arg("st") = 0, py::arg("stream") = 0);
    m.def("sum_f64", [](uintptr_t v, int64_t n, uintptr_t out, uintptr_t st, uintptr_t stream) {
        sart::launch_sum_f64(P<const double>(v), n, P<double>(out), P<const sart::SartState>(st), S(stream));
    }, py::arg("v"), py::arg("n"), py::arg("out"), py::arg("st") = 0, py::arg("stream") = 0);
    m.def("backproject64", [](uintptr_t A, int64_t ld, int64_t nrows, uintptr_t w, int nsplit, uintptr_t partial,
                              uintptr_t st, uintptr_t stream) {
        sart::launch_backproject64(P<const float>(A), ld, nrows, P<const double>(w), nsplit, P<double>(partial),
                                   P<const sart::SartState>(st), S(stream));
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("w"), py::arg("nsplit"), py::arg("partial"),
       py::arg("st") = 0, py::arg("stream") = 0);
    // fit64.hip: F [nv][ldf] = A X^T for nv <= 8 fp64 vectors X [nv][ldx] per pass over the shard (a
    // row or a column shard in its storage; rscale: an f16 shard's [nrows_pad] scales, then their inverses)
    m.def("fit64_group", &sart::fit64_group, py::arg("bf16") = false, py::arg("f16") = false,
          py::arg("sparse") = false);
    m.def("fit_forward", [](uintptr_t A, int64_t ld, int64_t nrows, int64_t nrows_pad, int64_t nvoxel, uintptr_t X,
                            int64_t ldx, int nv, uintptr_t F, int64_t ldf, uintptr_t stream, bool bf16, bool f16,
                            uintptr_t rscale) {
        sart::launch_fit64(P<const void>(A), bf16, f16, P<const float>(rscale), ld, nrows, nrows_pad, nvoxel,
                           P<const double>(X), ldx, nv, P<double>(F), ldf, S(stream));
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("nrows_pad"), py::arg("nvoxel"), py::arg("X"),
       py::arg("ldx"), py::arg("nv"), py::arg("F"), py::arg("ldf"), py::arg("stream") = 0, py::arg("bf16") = false,
       py::arg("f16") = false, py::arg("rscale") = 0);
    // sparse shard: the CSR arrays; Xt: ld x 8 doubles of scratch; lanes: lanes per row (0: a fixed 8)
    m.def("fit_forward_csr", [](uintptr_t row_ptr, uintptr_t col, uintptr_t val, int64_t nnz, int64_t nrows,
                                int64_t nvoxel, int64_t ld, uintptr_t X, int64_t ldx, int nv, uintptr_t Xt,
                                uintptr_t F, int64_t ldf, uintptr_t stream, int lanes) {
        sart::SparseRtm s;
        s.row_ptr = P<const int64_t>(row_ptr);
        s.col = P<const int32_t>(col);
        s.val = P<const float>(val);
        s.nnz = nnz;
        s.lanes_rows = lanes;
        sart::launch_fit64_csr(s, nrows, nvoxel, ld, P<const double>(X), ldx, nv, P<double>(Xt), P<double>(F), ldf,
                               S(stream));
    }, py::arg("row_ptr"), py::arg("col"), py::arg("val"), py::arg("nnz"), py::arg("nrows"), py::arg("nvoxel"),
       py::arg("ld"), py::arg("X"), py::arg("ldx"), py::arg("nv"), py::arg("Xt"), py::arg("F"), py::arg("ldf"),
       py::arg("stream") = 0, py::arg("lanes") = 0);
    // squared roughness norms of nv <= 8 fp64 solutions X [nv][ldx] under the Laplacian CSR (n rows); eta2: nv doubles,
    // scratch: rough64_scratch_elems(n) doubles
    m.def("rough64_scratch_elems", &sart::rough64_scratch_elems, py::arg("n"));
    m.def("rough64", [](uintptr_t row_ptr, uintptr_t col, uintptr_t val, int64_t n, uintptr_t X, int64_t ldx, int nv,
                        bool logx, uintptr_t eta2, uintptr_t scratch, uintptr_t stream) {
        sart::launch_rough64(P<const int64_t>(row_ptr), P<const int32_t>(col), P<const float>(val), n,
                             P<const double>(X), ldx, nv, logx, P<double>(eta2), P<double>(scratch), S(stream));
    }, py::arg("row_ptr"), py::arg("col"), py::arg("val"), py::arg("n"), py::arg("X"), py::arg("ldx"), py::arg("nv"),
       py::arg("logx"), py::arg("eta2"), py::arg("scratch"), py::arg("stream") = 0);
    // replicas r0 .. r0 + nrep - 1 (nrep <= 64) of the n device pixels g into out [nrep][ldo]; time_bits: the frame
    // time's IEEE-754 bits
    m.def("noise_replicas", [](uintptr_t g, int64_t n, uint64_t pixel0, uint64_t time_bits, uint32_t r0, int nrep,
                               double abs_, double shot, double rel, uint64_t seed, uintptr_t out, int64_t ldo,
                               uintptr_t stream) {
        sart::launch_noise_replicas(P<const double>(g), n, pixel0, time_bits, r0, nrep, abs_, shot, rel, seed,
                                    P<double>(out), ldo, S(stream));
    }, py::arg("g"), py::arg("n"), py::arg("pixel0"), py::arg("time_bits"), py::arg("r0"), py::arg("nrep"),
       py::arg("abs"), py::arg("shot"), py::arg("rel"), py::arg("seed"), py::arg("out"), py::arg("ldo"),
       py::arg("stream") = 0);
    // per-voxel mean and unbiased std over the rows of X [n][ldx] with use[r] != 0 (device uint8)
    m.def("moments64", [](uintptr_t X, int64_t ldx, int64_t nvoxel, int n, uintptr_t use, uintptr_t mean,
                          uintptr_t std_out, uintptr_t stream) {
        sart::launch_moments64(P<const double>(X), ldx, nvoxel, n, P<const uint8_t>(use), P<double>(mean),
                               P<double>(std_out), S(stream));
    }, py::arg("X"), py::arg("ldx"), py::arg("nvoxel"), py::arg("n"), py::arg("use"), py::arg("mean"), py::arg("std"),
       py::arg("stream") = 0);
    // ten doubles per column (sums [nv][10]) of nv <= 8 fp64 columns X [nv][ldx] against the truth t over nvoxel voxels;
    // scratch: phantom64_scratch_elems(nvoxel) doubles
    m.def("phantom64_scratch_elems", &sart::phantom64_scratch_elems, py::arg("nvoxel"));
    m.def("phantom64", [](uintptr_t X, int64_t ldx, int64_t nvoxel, int nv, uintptr_t t, uintptr_t sums,
                          uintptr_t scratch, uintptr_t stream) {
        sart::launch_phantom64(P<const double>(X), ldx, nvoxel, nv, P<const double>(t), P<double>(sums),
                               P<double>(scratch), S(stream));
    }, py::arg("X"), py::arg("ldx"), py::arg("nvoxel"), py::arg("nv"), py::arg("t"), py::arg("sums"),
       py::arg("scratch"), py::arg("stream") = 0);
    // hold-out sums (sums [n][ncam][6]) of n fp64 fitted images F [n][ldf] against the frame g: the pixels of camera m
    // are cam_start[m] .. cam_start[m + 1] - 1 (int64 [ncam + 1]), fold int32 per pixel, held int32 [n] (-1: none);
    // ldf >= cam_start[ncam] is the caller's to keep
    m.def("holdout64", [](uintptr_t F, int64_t ldf, int n, uintptr_t g, uintptr_t ell, double threshold, uintptr_t fold,
                          uintptr_t held, uintptr_t cam_start, int ncam, uintptr_t sums, uintptr_t stream) {
        sart::launch_holdout64(P<const double>(F), ldf, n, P<const double>(g), P<const double>(ell), threshold,
                               P<const int32_t>(fold), P<const int32_t>(held), P<const int64_t>(cam_start), ncam,
                               P<double>(sums), S(stream));
    }, py::arg("F"), py::arg("ldf"), py::arg("n"), py::arg("g"), py::arg("ell"), py::arg("threshold"), py::arg("fold"),
       py::arg("held"), py::arg("cam_start"), py::arg("ncam"), py::arg("sums"), py::arg("stream") = 0);
    m.def("prep_rows", [](uintptr_t g, int64_t nrows, int64_t nrows_pad, double inv_s, uintptr_t ray_length,
                          float len_thres, uintptr_t ghat, uintptr_t arow, uintptr_t gpos, uintptr_t wo,
                          uintptr_t stream) {
        sart::launch_prep_rows(P<const double>(g), nrows, nrows_pad, inv_s, P<const float>(ray_length), len_thres,
                               P<float>(ghat), P<float>(arow), P<float>(gpos), P<float>(wo), S(stream));
    });
    m.def("init_solution", [](uintptr_t x, int64_t n, int64_t n_pad, uintptr_t src_f32, uintptr_t src_f64,
                              double scale, uintptr_t stream) {
        sart::launch_init_solution(P<float>(x), n, n_pad, P<const float>(src_f32), P<const double>(src_f64), scale,
                                   S(stream));
    });
    m.def("penalty", [](bool logx, uintptr_t row_ptr, uintptr_t col, uintptr_t val, int64_t n, float beta,
                        uintptr_t x, uintptr_t pen, uintptr_t st, uintptr_t stream) {
        sart::launch_penalty(logx, P<const int64_t>(row_ptr), P<const int32_t>(col), P<const float>(val), n, beta,
                             P<const float>(x), P<float>(pen), P<const sart::SartState>(st), S(stream));
    });
    m.def("decide", [](uintptr_t st, uintptr_t Fslot, uintptr_t stream) {
        sart::launch_decide(P<sart::SartState>(st), P<const float>(Fslot), S(stream));
    });
    m.def("update_linear", [](uintptr_t x, uintptr_t d, uintptr_t pen, int64_t n, uintptr_t st, uintptr_t stream) {
        sart::launch_update_linear(P<float>(x), P<const float>(d), P<const float>(pen), n,
                                   P<const sart::SartState>(st), S(stream));
    });
    m.def("update_log", [](uintptr_t x, uintptr_t O, uintptr_t Fv, uintptr_t pen, float alpha, int64_t n,
                           uintptr_t st, uintptr_t stream) {
        sart::launch_update_log(P<float>(x), P<const float>(O), P<const float>(Fv), P<const float>(pen), alpha, n,
                                P<const sart::SartState>(st), S(stream));
    });
    m.def("state_begin", [](uintptr_t st, double G, double tol, int max_iter, uintptr_t stream) {
        sart::launch_state_begin(P<sart::SartState>(st), G, tol, max_iter, S(stream));
    });
    m.def("synth_matrix", [](uintptr_t A, int64_t ld, int64_t nrows_pad, int64_t nrows, int64_t ncols,
                             int64_t row_offset, uint64_t seed, float lo, float hi, uintptr_t stream,
                             int64_t col_offset, int64_t ncols_total) {
        sart::launch_synth_matrix_block(P<float>(A), ld, nrows_pad, nrows, ncols, row_offset, col_offset,
                                        ncols_total > 0 ? ncols_total : ncols, seed, lo, hi, S(stream));
    }, py::arg("A"), py::arg("ld"), py::arg("nrows_pad"), py::arg("nrows"), py::arg("ncols"), py::arg("row_offset"),
       py::arg("seed"), py::arg("lo"), py::arg("hi"), py::arg("stream"), py::arg("col_offset") = 0,
       py::arg("ncols_total") = 0);
    m.def("synth_vector", [](uintptr_t out, int64_t n, int64_t offset, uint64_t seed, double lo, double hi,
                             uintptr_t stream) {
        sart::launch_synth_vector(P<double>(out), n, offset, seed, lo, hi, S(stream));
    });
    m.def("fused_pick_k", &sart::fused_pick_k);
    m.def("fused_tile_rows", &sart::fused_tile_rows);
    m.def("fused_set_schedule", &sart::fused_set_schedule);
    m.def("fused_get_schedule", &sart::fused_get_schedule);
    m.def("fused_granules", &sart::fused_granules, py::arg("nrows_pad"), py::arg("J"), py::arg("xl") = true);
    m.def("fused_last_schedule", &sart::fused_last_schedule);
    m.def("fused_debug_map", &sart::fused_debug_map);
    m.def("fused_set_trace", [](uintptr_t buf, long long tiles) {
        sart::fused_set_trace(reinterpret_cast<unsigned long long*>(buf), tiles);
    });
    m.def("fused_set_debug", &sart::fused_set_debug);
    m.def("fused_debug_stats", &sart::fused_debug_stats);
    // one fp32 sweep on 8-KiB slabs in XCD-local row groups (variant 6: K = rows per tile) or variant 3, one chain
    m.def("fused_sweep", [](bool logmode, int K, int variant, uintptr_t A, int64_t ld, int64_t nrows, int64_t nrows_pad,
                            uintptr_t x, uintptr_t ghat, uintptr_t arow, uintptr_t partial, uintptr_t Fpart,
                            uintptr_t gran, int I, int J, uintptr_t st, uintptr_t xcnt, uintptr_t stream) {
        sart::FusedGeometry g;
        g.K = K, g.J = J, g.I = I, g.grid = I * J, g.variant = variant;
        const sart::FusedArgs a{P<const float>(A), nullptr, ld, nrows, nrows_pad, P<const float>(x), P<const float>(ghat),
                                P<const float>(arow), P<float>(partial), P<double>(Fpart), P<uint64_t>(gran), I, J,
                                P<sart::SartState>(st), P<unsigned>(xcnt)};
        sart::launch_fused_sweep(sart::fused_plan(g, sart::RtmStorage::f32, sart::FusedKnobs::current()), a, logmode,
                                 S(stream));
    });
    m.def("fused_min_bytes_from_env", &sart::fused_min_bytes_from_env);
    // The multi-frame MFMA projections: every direct kernel call plans from the environment as it is now
    // (MfKnobs::from_env(); the engine plans once, in its constructor)
    m.def("mf_forward_num_splits", &sart::mf_forward_num_splits, py::arg("ld"), py::arg("nrows_pad"), py::arg("target") = 0);
    m.def("mf_backproject_num_splits", &sart::mf_backproject_num_splits);
    m.def("mf_set_depth", &sart::mf_set_depth);
    m.def("mf_set_rows", &sart::mf_set_rows);
    m.def("mf_set_vox", &sart::mf_set_vox);
    m.def("mf_backproject_b16_num_splits", &sart::mf_backproject_b16_num_splits, py::arg("ld"), py::arg("nrows"),
          py::arg("a32") = false);
    m.def("mf_backproject_b16_vox_align", &sart::mf_backproject_b16_vox_align, py::arg("ld"), py::arg("a32") = false);
    auto key_dict = &mf_key_dict;
    // path: "fp32", "b16", "x3", "h16" or "s16"; nsplit 0: the planner's split count (what the engine allocates for)
    m.def("mf_plan_forward", [](const std::string& path, int nf, int64_t ld, int64_t nrows_pad, int nsplit) {
        return mf_fwd_plan_dict(sart::mf_plan_forward(sart::mf_path_from_name(path), nf, ld, nrows_pad,
                                                      sart::MfKnobs::from_env(), nsplit));
    }, py::arg("path"), py::arg("nf"), py::arg("ld"), py::arg("nrows_pad"), py::arg("nsplit") = 0);
    m.def("mf_plan_backproject", [](const std::string& path, int nf, int64_t ld, int64_t nrows, int nsplit) {
        return mf_bwd_plan_dict(sart::mf_plan_backproject(sart::mf_path_from_name(path), nf, ld, nrows,
                                                          sart::MfKnobs::from_env(), nsplit));
    }, py::arg("path"), py::arg("nf"), py::arg("ld"), py::arg("nrows"), py::arg("nsplit") = 0);
    // The engine plan of a shard under the environment as it is now (MfEngineKnobs::from_env, MfKnobs::from_env): what
    // a MultiFrameEngine built on the same inputs holds (MultiFrameEngine.plan). storage: "f32", "bf16" or "f16".
    m.def("mf_engine_plan", [](const std::string& storage, bool sparse, int64_t nnz, int frames, int64_t nrows,
                               int64_t nrows_pad, int64_t ld, int ranks, int mf_split_a, int check_interval) {
        return mf_engine_plan_dict(sart::mf_engine_plan(sart::rtm_storage_from_name(storage.c_str()), sparse, nnz,
                                                        frames, nrows, nrows_pad, ld, ranks, mf_split_a,
                                                        check_interval, sart::MfEngineKnobs::from_env()));
    }, py::arg("storage"), py::arg("sparse"), py::arg("nnz"), py::arg("frames"), py::arg("nrows"),
       py::arg("nrows_pad"), py::arg("ld"), py::arg("ranks") = 1, py::arg("mf_split_a") = -1,
       py::arg("check_interval") = 16);
    // the variant table's keys of one path and direction, each with the knob setting ("env") that selects it
    m.def("mf_variants", [key_dict](const std::string& path, int nf, bool forward) {
        py::list out;
        for (const sart::MfKey& k : sart::mf_variants(sart::mf_path_from_name(path), forward, nf)) {
            py::dict d = key_dict(k), env;
            for (const auto& kv : sart::mf_key_env(k)) env[py::str(kv.first)] = kv.second;
            d["env"] = env;
            out.append(d);
        }
        return out;
    }, py::arg("path"), py::arg("nf"), py::arg("forward") = true);
    auto fwd_plan = [](sart::MfPath path, int nf, int64_t ld, int64_t nrows_pad, int nsplit, const char* what) {
        if (nsplit < 1) throw std::runtime_error(std::string(what) + ": nsplit must be >= 1");
        return sart::mf_plan_forward(path, nf, ld, nrows_pad, sart::MfKnobs::from_env(), nsplit);
    };
    auto bwd_plan = [](sart::MfPath path, int nf, int64_t ld, int64_t nrows, int nsplit, const char* what) {
        if (nsplit < 1) throw std::runtime_error(std::string(what) + ": nsplit must be >= 1");
        return sart::mf_plan_backproject(path, nf, ld, nrows, sart::MfKnobs::from_env(), nsplit);
    };
    m.def("mf_forward", [fwd_plan](uintptr_t A, int64_t ld, int64_t nrows, int64_t nrows_pad, uintptr_t X, int64_t ldx,
                                   uintptr_t Fout, int nsplit, uintptr_t stream, int nf) {
        if (ldx != ld) throw std::runtime_error("mf_forward: ld must be a multiple of 64 and ldx == ld");
        sart::launch_mf_forward(fwd_plan(sart::MfPath::fp32, nf, ld, nrows_pad, nsplit, "mf_forward"),
                                P<const float>(A), nrows, P<const float>(X), P<float>(Fout), S(stream));
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("nrows_pad"), py::arg("X"), py::arg("ldx"),
       py::arg("Fout"), py::arg("nsplit"), py::arg("stream"), py::arg("nf") = 16);
    m.def("mf_forward_x3", [fwd_plan](uintptr_t A, int64_t ld, int64_t nrows, int64_t nrows_pad, uintptr_t Xh,
                                      uintptr_t Xl, uintptr_t Fout, int nsplit, uintptr_t stream, int nf, bool xblk) {
        sart::launch_mf_forward_x3(fwd_plan(sart::MfPath::x3, nf, ld, nrows_pad, nsplit, "mf_forward_x3"),
                                   P<const float>(A), nrows, P<const sart::bf16_t>(Xh), P<const sart::bf16_t>(Xl),
                                   P<float>(Fout), S(stream), xblk);
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("nrows_pad"), py::arg("Xh"), py::arg("Xl"),
       py::arg("Fout"), py::arg("nsplit"), py::arg("stream"), py::arg("nf"), py::arg("xblk") = false);
    m.def("mf_backproject_x3", [bwd_plan](uintptr_t A, int64_t ld, int64_t nrows, uintptr_t Wh, uintptr_t Wl,
                                          int64_t ldw, int nsplit, uintptr_t partial, uintptr_t stream, int nf,
                                          int64_t v0, int64_t v1) {
        sart::launch_mf_backproject_x3(bwd_plan(sart::MfPath::x3, nf, ld, nrows, nsplit, "mf_backproject_x3"),
                                       P<const float>(A), P<const sart::bf16_t>(Wh), P<const sart::bf16_t>(Wl), ldw,
                                       P<float>(partial), S(stream), v0, v1);
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("Wh"), py::arg("Wl"), py::arg("ldw"), py::arg("nsplit"),
       py::arg("partial"), py::arg("stream"), py::arg("nf") = 16, py::arg("v0") = 0, py::arg("v1") = -1);
    m.def("mf_split_x", [](uintptr_t X, int64_t n, uintptr_t hi, uintptr_t lo, uintptr_t stream, bool perm,
                           int64_t ld) {
        sart::launch_mf_split_x(P<const float>(X), n, P<sart::bf16_t>(hi), P<sart::bf16_t>(lo), S(stream), perm, ld);
    }, py::arg("X"), py::arg("n"), py::arg("hi"), py::arg("lo"), py::arg("stream"), py::arg("perm") = false,
       py::arg("ld") = 0);
    m.def("mf_split_w16", [](uintptr_t W, int64_t nrows_pad, int nf, int64_t ldw, uintptr_t w1, uintptr_t w2,
                             uintptr_t wmax, float a_scale, uintptr_t inv_scale, uintptr_t stream) {
        sart::launch_mf_split_w16(P<const float>(W), nrows_pad, nf, ldw, P<uint16_t>(w1), P<uint16_t>(w2),
                                  P<unsigned>(wmax), a_scale, P<float>(inv_scale), S(stream));
    });
    m.def("absmax_pow2_scale", [](uintptr_t A, int64_t n, uintptr_t scratch, uintptr_t stream) {
        return sart::absmax_pow2_scale(P<const float>(A), n, P<unsigned>(scratch), S(stream));
    });
    m.def("mf_backproject_h16", [bwd_plan](uintptr_t A, int64_t ld, int64_t nrows, uintptr_t W1, uintptr_t W2,
                                           int64_t ldw, int nsplit, uintptr_t partial, uintptr_t stream, int nf,
                                           int64_t v0, int64_t v1, uintptr_t csc, uintptr_t inv_scale) {
        sart::launch_mf_backproject_h16(bwd_plan(sart::MfPath::h16, nf, ld, nrows, nsplit, "mf_backproject_h16"),
                                        P<const float>(A), P<const uint16_t>(W1), P<const uint16_t>(W2), ldw,
                                        P<float>(partial), S(stream), v0, v1, P<const float>(csc),
                                        P<const float>(inv_scale));
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("W1"), py::arg("W2"), py::arg("ldw"), py::arg("nsplit"),
       py::arg("partial"), py::arg("stream"), py::arg("nf"), py::arg("v0"), py::arg("v1"), py::arg("csc"),
       py::arg("inv_scale"));
    m.def("mf_row_scales", [](uintptr_t A, int64_t ld, int64_t nrows_pad, uintptr_t rsc, uintptr_t stream) {
        sart::launch_mf_row_scales(P<const float>(A), ld, nrows_pad, P<float>(rsc), S(stream));
    });
    m.def("mf_col_scales", [](uintptr_t A, int64_t ld, int64_t nrows_pad, uintptr_t scratch, uintptr_t csc,
                              uintptr_t stream) {
        sart::launch_mf_col_scales(P<const float>(A), ld, nrows_pad, P<unsigned>(scratch), P<float>(csc), S(stream));
    });
    m.def("mf_split_x16", [](uintptr_t X, int64_t ld, int nf, uintptr_t x1, uintptr_t x2, uintptr_t xmax,
                             uintptr_t xinv, uintptr_t stream, bool perm, bool blocked) {
        sart::launch_mf_split_x16(P<const float>(X), ld, nf, P<uint16_t>(x1), P<uint16_t>(x2), P<unsigned>(xmax),
                                  P<float>(xinv), S(stream), perm, blocked);
    }, py::arg("X"), py::arg("ld"), py::arg("nf"), py::arg("x1"), py::arg("x2"), py::arg("xmax"), py::arg("xinv"),
       py::arg("stream"), py::arg("perm") = true, py::arg("blocked") = false);
    m.def("mf_forward_h16", [fwd_plan](uintptr_t A, int64_t ld, int64_t nrows, int64_t nrows_pad, uintptr_t X1,
                                       uintptr_t X2, uintptr_t Fout, int nsplit, uintptr_t stream, int nf, bool xblk,
                                       uintptr_t rsc, uintptr_t xinv) {
        sart::launch_mf_forward_h16(fwd_plan(sart::MfPath::h16, nf, ld, nrows_pad, nsplit, "mf_forward_h16"),
                                    P<const float>(A), nrows, P<const uint16_t>(X1), P<const uint16_t>(X2),
                                    P<float>(Fout), S(stream), xblk, P<const float>(rsc), P<const float>(xinv));
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("nrows_pad"), py::arg("X1"), py::arg("X2"),
       py::arg("Fout"), py::arg("nsplit"), py::arg("stream"), py::arg("nf"), py::arg("xblk"), py::arg("rsc"),
       py::arg("xinv"));
    m.def("mf_forward_s16", [fwd_plan](uintptr_t A, int64_t ld, int64_t nrows, int64_t nrows_pad, uintptr_t X1,
                                       uintptr_t X2, uintptr_t Fout, int nsplit, uintptr_t stream, int nf, bool xblk,
                                       uintptr_t rsc, uintptr_t xinv) {
        sart::launch_mf_forward_s16(fwd_plan(sart::MfPath::s16, nf, ld, nrows_pad, nsplit, "mf_forward_s16"),
                                    P<const sart::f16s_t>(A), nrows, P<const uint16_t>(X1), P<const uint16_t>(X2),
                                    P<float>(Fout), S(stream), xblk, P<const float>(rsc), P<const float>(xinv));
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("nrows_pad"), py::arg("X1"), py::arg("X2"),
       py::arg("Fout"), py::arg("nsplit"), py::arg("stream"), py::arg("nf"), py::arg("xblk"), py::arg("rsc"),
       py::arg("xinv"));
    m.def("mf_backproject_s16", [bwd_plan](uintptr_t A, int64_t ld, int64_t nrows, uintptr_t W1, uintptr_t W2,
                                           int64_t ldw, int nsplit, uintptr_t partial, uintptr_t stream, int nf,
                                           int64_t v0, int64_t v1, uintptr_t inv_scale) {
        sart::launch_mf_backproject_s16(bwd_plan(sart::MfPath::s16, nf, ld, nrows, nsplit, "mf_backproject_s16"),
                                        P<const sart::f16s_t>(A), P<const uint16_t>(W1), P<const uint16_t>(W2), ldw,
                                        P<float>(partial), S(stream), v0, v1, P<const float>(inv_scale));
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("W1"), py::arg("W2"), py::arg("ldw"), py::arg("nsplit"),
       py::arg("partial"), py::arg("stream"), py::arg("nf"), py::arg("v0"), py::arg("v1"), py::arg("inv_scale"));
    m.def("mf_scale_w_rows", [](uintptr_t W, uintptr_t rinv, int64_t nrows_pad, int nf, uintptr_t out,
                                uintptr_t stream) {
        sart::launch_mf_scale_w_rows(P<const float>(W), P<const float>(rinv), nrows_pad, nf, P<float>(out), S(stream));
    });
    m.def("mf_split_w", [](uintptr_t W, int64_t nrows_pad, int nf, int64_t ldw, uintptr_t hi, uintptr_t lo,
                           uintptr_t stream, bool three) {
        sart::launch_mf_split_w(P<const float>(W), nrows_pad, nf, ldw, P<sart::bf16_t>(hi), P<sart::bf16_t>(lo),
                                S(stream), three);
    }, py::arg("W"), py::arg("nrows_pad"), py::arg("nf"), py::arg("ldw"), py::arg("hi"), py::arg("lo"),
       py::arg("stream"), py::arg("three") = false);
    m.def("mf_forward_b16", [fwd_plan](uintptr_t A, int64_t ld, int64_t nrows, int64_t nrows_pad, uintptr_t Xh,
                                       uintptr_t Xl, uintptr_t Fout, int nsplit, uintptr_t stream, int nf, bool xblk) {
        sart::launch_mf_forward_b16(fwd_plan(sart::MfPath::b16, nf, ld, nrows_pad, nsplit, "mf_forward_b16"),
                                    P<const sart::bf16_t>(A), nrows, P<const sart::bf16_t>(Xh),
                                    P<const sart::bf16_t>(Xl), P<float>(Fout), S(stream), xblk);
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("nrows_pad"), py::arg("Xh"), py::arg("Xl"),
       py::arg("Fout"), py::arg("nsplit"), py::arg("stream"), py::arg("nf"), py::arg("xblk") = false);
    m.def("mf_backproject_b16", [bwd_plan](uintptr_t A, int64_t ld, int64_t nrows, uintptr_t Wh, uintptr_t Wl,
                                           int64_t ldw, int nsplit, uintptr_t partial, uintptr_t stream, int nf,
                                           int64_t v0, int64_t v1) {
        sart::launch_mf_backproject_b16(bwd_plan(sart::MfPath::b16, nf, ld, nrows, nsplit, "mf_backproject_b16"),
                                        P<const sart::bf16_t>(A), P<const sart::bf16_t>(Wh),
                                        P<const sart::bf16_t>(Wl), ldw, P<float>(partial), S(stream), v0, v1);
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("Wh"), py::arg("Wl"), py::arg("ldw"), py::arg("nsplit"),
       py::arg("partial"), py::arg("stream"), py::arg("nf") = 16, py::arg("v0") = 0, py::arg("v1") = -1);
    m.def("mf_backproject", [bwd_plan](uintptr_t A, int64_t ld, int64_t nrows, uintptr_t W, int nsplit,
                                       uintptr_t partial, uintptr_t stream, int nf) {
        sart::launch_mf_backproject(bwd_plan(sart::MfPath::fp32, nf, ld, nrows, nsplit, "mf_backproject"),
                                    P<const float>(A), P<const float>(W), P<float>(partial), S(stream));
    }, py::arg("A"), py::arg("ld"), py::arg("nrows"), py::arg("W"), py::arg("nsplit"), py::arg("partial"),
       py::arg("stream"), py::arg("nf") = 16);
}
