// Python bindings of the native runtime: rocmdash._native.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <memory>
#include <stdexcept>

#include "device_window.h"
#include "frame_render.h"
#include "long_window.h"
#include "node_window.h"
#include "publish.h"
#include "rccl_comm.h"
#include "long_window_buckets.h"
#include "window_autocorr.h"
#include "window_buckets.h"
#include "window_excursions.h"
#include "window_heatmap.h"
#include "window_joint.h"
#include "window_periods.h"
#include "window_quantiles.h"
#include "window_trend.h"
#include "window_xcorr.h"

namespace rocmdash {
int launch_spin(uint32_t workgroups, double us, void* stream);  // calib.hip
int launch_gather32(const void* src, uint64_t src_bytes, void* out, uint64_t out_bytes, uint32_t threads,
                    uint32_t seed, void* stream);
int launch_store64(void* dst, uint64_t dst_bytes, uint32_t threads, void* stream);
int launch_store32(void* dst, uint64_t dst_bytes, uint32_t threads, void* stream);
}  // namespace rocmdash
#include "ring.h"
#include "node_counters.h"
#include "sampler.h"
#include "sources.h"
#include "window_stats.h"

namespace py = pybind11;
using namespace rocmdash;

namespace {

py::dict info_dict(const GpuInfo& g) {
  py::dict d;
  d["index"] = g.index;
  d["bdf"] = g.bdf;
  d["model_number"] = g.model_number;
  d["product_name"] = g.product_name;
  d["market_name"] = g.market_name;
  d["power_limit_w"] = g.power_limit_w;
  d["vram_total_mb"] = g.vram_total_mb;
  d["edge_is_hotspot"] = g.edge_is_hotspot;
  d["metrics_path"] = g.metrics_path;
  d["metrics_table"] = g.metrics_table;
  d["metrics_calibration"] = g.metrics_calibration;
  return d;
}

py::list names(const char* const* n) {
  py::list l;
  for (; *n; ++n) l.append(*n);
  return l;
}

}  // namespace

PYBIND11_MODULE(_native, m) {
  m.doc() = "rocmdash native runtime: rings, samplers (amd-smi, rocprofiler-sdk), HIP window stats";

  m.attr("SMI_FIELDS") = names(smi_field_names());
  m.attr("CTR_FIELDS") = names(ctr_field_names());
  m.attr("STAT_NAMES") = py::make_tuple("min", "max", "mean", "p0", "p1", "p2", "last", "count");
  m.attr("MAX_SERIES_PER_LAUNCH") = int(kMaxSeriesPerLaunch);

  py::class_<SeriesRing, std::shared_ptr<SeriesRing>>(m, "SeriesRing")
      .def(py::init<uint32_t, uint64_t>(), py::arg("width"), py::arg("capacity"))
      .def_property_readonly("width", &SeriesRing::width)
      .def_property_readonly("capacity", &SeriesRing::capacity)
      .def_property_readonly("pinned", &SeriesRing::pinned)
      .def_property_readonly("head", &SeriesRing::head)
      .def_property_readonly("last_timestamp", &SeriesRing::last_timestamp)
      .def_property_readonly("rows_ptr", [](const SeriesRing& r) { return reinterpret_cast<uintptr_t>(r.rows()); })
      .def(
          "push",
          [](SeriesRing& r, py::array_t<float, py::array::c_style | py::array::forcecast> row, uint64_t t_ns) {
            if (row.size() != r.width()) throw std::invalid_argument("row size != ring width");
            r.push(row.data(), t_ns);
          },
          py::arg("row"), py::arg("t_ns"))
      .def(
          "push_many",
          [](SeriesRing& r, py::array_t<float, py::array::c_style | py::array::forcecast> rows,
             py::array_t<uint64_t, py::array::c_style | py::array::forcecast> ts) {
            if (rows.ndim() != 2 || rows.shape(1) != r.width() || ts.size() != rows.shape(0))
              throw std::invalid_argument("rows must be [n, width] with n timestamps");
            for (py::ssize_t i = 0; i < rows.shape(0); ++i) r.push(rows.data(i, 0), ts.data()[i]);
          },
          py::arg("rows"), py::arg("ts"))
      .def(
          "window",
          [](const SeriesRing& r, uint64_t n) {
            py::array_t<float> rows({py::ssize_t(n), py::ssize_t(r.width())});
            py::array_t<uint64_t> ts{py::ssize_t(n)};
            uint64_t got;
            {
              py::gil_scoped_release nogil;
              got = r.read_window(n, rows.mutable_data(), ts.mutable_data());
            }
            rows.resize({py::ssize_t(got), py::ssize_t(r.width())});
            ts.resize({py::ssize_t(got)});
            return py::make_tuple(rows, ts);
          },
          py::arg("n"), "Newest <= n rows (oldest first) and their timestamps; torn rows dropped.");

  py::class_<Source, std::shared_ptr<Source>>(m, "Source")
      .def_property_readonly("width", &Source::width)
      .def_property_readonly("kind", &Source::kind)
      .def_property_readonly("backend", &Source::backend)
      .def("info", [](const Source& s) { return info_dict(s.info()); })
      .def("counts", [](const Source& s) {
        py::dict d;
        for (const auto& kv : s.counts()) d[py::str(kv.first)] = kv.second;
        return d;
      })
      .def("xcd_detail", [](const Source& s) -> py::object {
        const std::vector<float> v = s.xcd_detail();
        if (v.empty()) return py::none();
        const py::ssize_t n = py::ssize_t(v.size() / 2);
        py::array_t<float> busy{n}, clk{n};
        std::memcpy(busy.mutable_data(), v.data(), sizeof(float) * size_t(n));
        std::memcpy(clk.mutable_data(), v.data() + n, sizeof(float) * size_t(n));
        py::dict d;
        d["busy"] = busy;
        d["clock_mhz"] = clk;
        return d;
      }, "Per-XCD busy (%) and gfx clock (MHz) of the last sample, or None")
      .def("set_back_to_back", &Source::set_back_to_back, py::arg("on"),
           "Hint that sample() is being polled back to back (what Sampler.start_free sets).")
      .def("sample", [](Source& s) -> py::object {
        py::array_t<float> row{py::ssize_t(s.width())};
        bool ok;
        {
          py::gil_scoped_release nogil;
          ok = s.sample(row.mutable_data());
        }
        if (!ok) return py::none();
        return row;
      });

  m.def("make_synthetic_source", &make_synthetic_source, py::arg("kind"), py::arg("seed"),
        py::arg("total_vram_mb") = 294896.0);
  m.def("make_smi_source", &make_smi_source, py::arg("bdf") = 0, py::arg("index") = 0);
  m.def("make_counter_source", &make_counter_source, py::arg("bdf") = 0, py::arg("index") = 0);
  m.def("make_counter_source_all", &make_counter_source_all, py::arg("bdf") = 0, py::arg("index") = 0,
        "Counters of the whole physical GPU at this PCI address (every compute partition combined).");
  m.def("amdsmi_gpu_count", &amdsmi_gpu_count);
  m.def("amdsmi_enumerate", []() {
    py::list l;
    for (auto& g : amdsmi_enumerate()) l.append(info_dict(g));
    return l;
  });
  m.def("counters_preinit", &counters_preinit, py::arg("counter_names"), py::arg("only_ordinal") = -1,
        py::arg("only_bdf") = 0);
  m.def("make_null_source", &make_null_source, py::arg("kind"));
  m.def(
      "make_shm_source",
      [](const std::string& path, double hz, const std::string& kind) -> std::shared_ptr<Source> {
        return std::make_shared<ShmSource>(path, hz, kind);
      },
      py::arg("path"), py::arg("hz"), py::arg("kind") = "counter",
      "A rank's view of its GPU's rows published by the node's counter process (shm_ring.h).");
  py::class_<ShmPublisher, std::shared_ptr<ShmPublisher>>(
      m, "ShmPublisher", "The node counter process's publisher: one lane (thread) per GPU source -> its shm ring.")
      .def(py::init<const std::vector<std::string>&, std::vector<std::shared_ptr<Source>>, double, uint64_t>(),
           py::arg("paths"), py::arg("sources"), py::arg("hz"), py::arg("capacity") = 4096)
      .def("start", &ShmPublisher::start)
      .def("stop", &ShmPublisher::stop, py::arg("grace_s") = 2.0, py::call_guard<py::gil_scoped_release>())
      .def("replace", &ShmPublisher::replace, py::arg("lane"), py::arg("source"),
           "Abandon lane i and start a fresh one with `source` and a new ring file; returns its generation.")
      .def("stats", &ShmPublisher::stats,
           "per ring: [samples, failures, mean read us, last read us, beat age s, lane generation, in-read s]");
  m.def("make_hanging_source", &make_hanging_source, py::arg("inner"), py::arg("after_s"),
        "Fault injection: a source whose reads block forever `after_s` seconds after its first read.");
  m.def(
      "make_replay_source",
      [](const std::string& kind, py::array_t<float, py::array::c_style | py::array::forcecast> rows, py::dict info) {
        if (rows.ndim() != 2) throw std::invalid_argument("rows must be [n, width]");
        std::vector<float> v(rows.data(), rows.data() + rows.size());
        GpuInfo g;
        if (info.contains("index")) g.index = info["index"].cast<int>();
        if (info.contains("bdf")) g.bdf = info["bdf"].cast<uint64_t>();
        if (info.contains("model_number")) g.model_number = info["model_number"].cast<std::string>();
        if (info.contains("product_name")) g.product_name = info["product_name"].cast<std::string>();
        if (info.contains("market_name")) g.market_name = info["market_name"].cast<std::string>();
        if (info.contains("power_limit_w")) g.power_limit_w = info["power_limit_w"].cast<double>();
        if (info.contains("vram_total_mb")) g.vram_total_mb = info["vram_total_mb"].cast<double>();
        return make_replay_source(kind, v, uint32_t(rows.shape(1)), g);
      },
      py::arg("kind"), py::arg("rows"), py::arg("info") = py::dict());
  py::class_<RawCalibrationPolicy>(m, "RawCalibrationPolicy",
                                    "The SMI source's raw SMU-table calibration / retry policy (CPU-testable).")
      .def(py::init<double, int, int>(), py::arg("retry_s") = 60.0, py::arg("need") = 6, py::arg("trials") = 8)
      .def("due", &RawCalibrationPolicy::due, py::arg("now_ns"))
      .def("record", &RawCalibrationPolicy::record, py::arg("matched"), py::arg("now_ns"), py::arg("final") = false)
      .def_property_readonly("raw", &RawCalibrationPolicy::raw)
      .def_property_readonly("final_refusal", &RawCalibrationPolicy::final_refusal)
      .def_property_readonly("attempts", &RawCalibrationPolicy::attempts)
      .def_property_readonly("promotions", &RawCalibrationPolicy::promotions)
      .def_property_readonly("last_matched", &RawCalibrationPolicy::last_matched);
  py::class_<SmuTableTracker>(m, "SmuTableTracker",
                              "When the SMI source reads the SMU table while polled back to back (CPU-testable).")
      .def(py::init<int64_t, int64_t>(), py::arg("guard_ns") = kSmuGuardNs, py::arg("hard_ns") = kSmuHardNs)
      .def("set_back_to_back", &SmuTableTracker::set_back_to_back, py::arg("on"))
      .def("restart", &SmuTableTracker::restart)
      .def("should_read", &SmuTableTracker::should_read, py::arg("now_ns"))
      .def("record", &SmuTableTracker::record, py::arg("now_ns"), py::arg("changed"), py::arg("fw_ts") = 0)
      .def_property_readonly("state", [](const SmuTableTracker& t) { return int(t.state()); })
      .def_property_readonly("period_ns", &SmuTableTracker::period_ns)
      .def_property_readonly("guard_ns", &SmuTableTracker::guard_ns)
      .def_property_readonly("hard_ns", &SmuTableTracker::hard_ns)
      .def_property_readonly("changes", &SmuTableTracker::changes)
      .def_property_readonly("locks", &SmuTableTracker::locks)
      .def_property_readonly("resyncs", &SmuTableTracker::resyncs)
      .def_property_readonly("missed", &SmuTableTracker::missed);
  m.attr("SMU_GUARD_NS") = kSmuGuardNs;
  m.attr("SMU_HARD_NS") = kSmuHardNs;
  m.def("counters_ready", &counters_ready);
  m.def("counters_status", &counters_status);

  py::class_<Sampler, std::shared_ptr<Sampler>>(m, "Sampler")
      .def(py::init<std::shared_ptr<Source>, std::shared_ptr<SeriesRing>, double>(), py::arg("source"),
           py::arg("ring"), py::arg("hz"))
      .def("start", &Sampler::start)
      .def("start_free", &Sampler::start_free, py::arg("max_hz") = 50000.0)
      .def("calls", &Sampler::calls)
      .def("last_start_ns", &Sampler::last_start_ns)
      .def("wait_calls", &Sampler::wait_calls, py::arg("target"), py::arg("timeout_s"),
           py::call_guard<py::gil_scoped_release>())
      .def("stop", &Sampler::stop, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("running", &Sampler::running)
      .def_property_readonly("hz", &Sampler::hz)
      .def_property_readonly("ring", &Sampler::ring)
      .def_property_readonly("source", &Sampler::source)
      .def("sample_once", &Sampler::sample_once, py::call_guard<py::gil_scoped_release>())
      .def("request", &Sampler::request, py::call_guard<py::gil_scoped_release>())
      .def("wait", &Sampler::wait, py::call_guard<py::gil_scoped_release>())
      .def("stats", [](const Sampler& s) {
        auto st = s.stats();
        py::dict d;
        d["samples"] = st.samples;
        d["failures"] = st.failures;
        d["overruns"] = st.overruns;
        d["last_us"] = st.last_us;
        d["max_us"] = st.max_us;
        d["mean_us"] = st.mean_us;
        d["p50_us"] = st.p50_us;
        d["p99_us"] = st.p99_us;
        return d;
      })
      .def("recent_us", &Sampler::recent_us)
      .def("counts", [](const Sampler& s) {
        const auto st = s.counts();
        return py::make_tuple(st.samples, st.failures, st.overruns);
      })
      .def("set_affinity", &Sampler::set_affinity, py::arg("cpus"))
      .def("set_spin_us", &Sampler::set_spin_us, py::arg("us"));

  m.def("long_window_chunk_plan", &long_window_chunk_plan, py::arg("window"), py::arg("widths"), py::arg("cus") = 256,
        py::arg("chunk_rows") = 0, py::arg("rounds") = 1,
        "per ring (rows per workgroup, workgroups per segment) of the long-window passes");
  m.def("long_window_node_cap", &long_window_node_cap, py::arg("maxmid"), py::arg("nranks"),
        "node bracket records: the next refresh's key cap from the node's most kept keys");
  // for the CPU tests only (tests/test_lw_worklist.py): the incremental pass B's work list and
  // its shaping as LongWindowSet computes them; not an interface of the service
  m.attr("LONG_WINDOW_NEVER") = kLongNever;
  m.def(
      "long_window_work_list",
      [](uint32_t window, const std::vector<std::array<uint64_t, 4>>& rings, std::vector<uint64_t> seg_head,
         const std::vector<uint32_t>& want, const std::vector<uint32_t>& changed) {
        std::vector<LwWorkRing> rs;
        size_t series = 0, segs = 0;
        for (const auto& r : rings) {
          if (r[0] == 0 || r[0] > uint64_t(kLongMaxWidth) || r[1] == 0 || r[2] == 0)
            throw std::invalid_argument("long_window_work_list: rings are (width 1..16, chunk_rows, nchunks, copied)");
          rs.push_back(LwWorkRing{uint32_t(r[0]), uint32_t(r[1]), uint32_t(r[2]), r[3]});
          series += r[0];
          segs += (r[0] + 7) / 8;
        }
        if (window == 0 || (window & (window - 1)) || seg_head.size() < segs || want.size() != series ||
            changed.size() != series)
          throw std::invalid_argument("long_window_work_list: a power-of-two window, a head per segment, flags per series");
        auto work = long_window_work_list(window, rs.data(), rs.size(), seg_head.data(), want.data(), changed.data());
        return py::make_tuple(work, seg_head);
      },
      py::arg("window"), py::arg("rings"), py::arg("seg_head"), py::arg("want"), py::arg("changed"),
      "test hook: (the (segment << 20 | chunk) list pass B streams, the updated segment heads)");
  m.def(
      "long_window_shape_work",
      [](const std::vector<uint32_t>& work, const std::vector<uint32_t>& seg_cols, uint32_t flat_grid,
         uint32_t fuse_chunks, size_t split_max, bool fuse) {
        for (uint32_t e : work)
          if ((e >> 20) >= seg_cols.size()) throw std::invalid_argument("long_window_shape_work: segment out of range");
        const LwWorkShape sh = long_window_shape_work(work, seg_cols, flat_grid, fuse_chunks, split_max, fuse);
        return py::make_tuple(sh.pass, sh.fused, sh.colsplit, sh.grid);
      },
      py::arg("work"), py::arg("seg_cols"), py::arg("flat_grid"), py::arg("fuse_chunks"), py::arg("split_max"),
      py::arg("fuse"), "test hook: (pass B's list, the fused list, colsplit, pass B's grid)");
  py::class_<LongWindowSet, std::shared_ptr<LongWindowSet>>(m, "LongWindowSet")
      .def(py::init<uint32_t, int, bool, uint32_t>(), py::arg("window"), py::arg("device"), py::arg("use_graph") = false,
           py::arg("chunk_rows") = 0)
      .def_property_readonly("chunk_rows", &LongWindowSet::chunk_rows)
      .def_property_readonly("chunk_plan", &LongWindowSet::chunk_plan)
      .def_property("brackets", &LongWindowSet::brackets, &LongWindowSet::set_brackets)
      .def_property("incremental", &LongWindowSet::incremental, &LongWindowSet::set_incremental,
                    "incremental bracket mode: pass B streams only the chunks new rows landed in (A/B switch)")
      .def_property("fused_passb", &LongWindowSet::fused_passb, &LongWindowSet::set_fused_passb,
                    "a short incremental work list: scan B streams the changed chunks itself, one kernel (A/B switch)")
      .def("bracket_stats", &LongWindowSet::bracket_stats, py::arg("mode") = 0,
           "Per series [refreshes, hits, last refresh hit] of the local (0) or node (1) brackets")
      .def(
          "bracket_state",
          [](const LongWindowSet& w, int mode) {
            py::list out;
            for (const auto& r : w.bracket_state(mode)) {
              py::dict d;
              py::list lo, hi, delta, cin;
              for (int q = 0; q < 3; ++q) {
                lo.append(r[q]);
                hi.append(r[3 + q]);
                float f;
                std::memcpy(&f, &r[6 + q], 4);
                delta.append(f);
                cin.append(r[9 + q]);
              }
              d["lo"] = lo;
              d["hi"] = hi;
              d["delta"] = delta;
              d["cin"] = cin;
              d["valid"] = r[12];
              d["nounion"] = r[13];
              d["hit"] = r[15];
              d["refreshes"] = r[16];
              d["hits"] = r[17];
              out.append(d);
            }
            return out;
          },
          py::arg("mode") = 0, "Every series' bracket record (keys as uint32 order keys, delta in value units)")
      .def_property("wave_private_level", &LongWindowSet::wave_private_level,
                    &LongWindowSet::set_wave_private_level)
      .def_property("wave_private", &LongWindowSet::wave_private, &LongWindowSet::set_wave_private,
                    "pass 0: per-wave LDS histogram copies for 8-bit digits (A/B switch)")
      .def_property("prefetch", &LongWindowSet::prefetch, &LongWindowSet::set_prefetch,
                    "load the next iteration's rows while counting this one's (A/B switch)")
      .def_property("brk_target", &LongWindowSet::brk_target, &LongWindowSet::set_brk_target,
                    "samples a local bracket aims to hold (256..2048)")
      .def("set_phase_clocks", &LongWindowSet::set_phase_clocks, py::arg("on"))
      .def("phase_clocks", &LongWindowSet::phase_clocks)
      .def_property("plan_rounds", &LongWindowSet::plan_rounds, &LongWindowSet::set_plan_rounds,
                    "rounds of the chip's workgroup slots a planned full pass takes (before the first refresh)")
      .def_property("compact", &LongWindowSet::compact, &LongWindowSet::set_compact,
                    "pass 2 keeps the keys it counts and pass 3 reads only those (A/B switch)")
      .def("add_ring", &LongWindowSet::add_ring, py::arg("ring"))
      .def_property_readonly("num_series", &LongWindowSet::num_series)
      .def_property_readonly("window", &LongWindowSet::window)
      .def(
          "refresh",
          [](LongWindowSet& w, uintptr_t out, uintptr_t stream, float p0, float p1, float p2) {
            py::gil_scoped_release nogil;
            w.refresh(reinterpret_cast<float*>(out), reinterpret_cast<void*>(stream), p0, p1, p2);
          },
          py::arg("out_ptr"), py::arg("stream"), py::arg("p0") = 50.0f, py::arg("p1") = 90.0f, py::arg("p2") = 99.0f)
      .def(
          "export_trend",
          [](LongWindowSet& w, uint32_t P, uintptr_t dst, uintptr_t stream) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_trend(P, reinterpret_cast<float*>(dst), reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_trend failed: " + std::to_string(e));
          },
          py::arg("columns"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue every series' window trend after the last refresh: dst [S][columns + 1][4] floats "
          "(min, max, mean, count per slot of window / columns rows).")
      .def(
          "export_quantiles",
          [](LongWindowSet& w, uint32_t P, uintptr_t dst, uintptr_t stream, float p0, float p1, float p2) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_quantiles(P, p0, p1, p2, reinterpret_cast<float*>(dst), reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_quantiles failed: " + std::to_string(e));
          },
          py::arg("columns"), py::arg("dst_ptr"), py::arg("stream"), py::arg("p0") = 50.0f, py::arg("p1") = 90.0f,
          py::arg("p2") = 99.0f,
          "Enqueue every series' window quantile trend after the last refresh: dst [S][columns + 1][4] floats "
          "(the three percentiles and the count per slot of window / columns rows).")
      .def(
          "export_autocorr",
          [](LongWindowSet& w, uint32_t span, uintptr_t scale, uint32_t L, uintptr_t dst, uintptr_t stream) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_autocorr(span, reinterpret_cast<const float*>(scale), L, reinterpret_cast<int64_t*>(dst),
                                    reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_autocorr failed: " + std::to_string(e));
          },
          py::arg("span"), py::arg("scale_ptr"), py::arg("lags"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue every series' autocorrelation sums over the newest min(n, span) rows after the last refresh: scale "
          "[S] floats -> dst [S][lags + 1][4] int64 (n, Sx, Sy, Sxy per lag).")
      .def(
          "export_periods",
          [](LongWindowSet& w, uint32_t span, uint32_t P, uintptr_t scale, uint32_t L, uintptr_t dst, uintptr_t stream) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_periods(span, P, reinterpret_cast<const float*>(scale), L, reinterpret_cast<int64_t*>(dst),
                                   reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_periods failed: " + std::to_string(e));
          },
          py::arg("span"), py::arg("columns"), py::arg("scale_ptr"), py::arg("lags"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue every series' window period trend after the last refresh: the autocorrelation's sums per trend slot of "
          "the newest min(n, span) rows: scale [S] floats -> dst [S][columns + 1][lags + 1][4] int64.")
      .def(
          "export_xcorr",
          [](LongWindowSet& w, const std::vector<std::pair<uint32_t, uint32_t>>& pairs, uint32_t span, uintptr_t scale,
             uint32_t L, uintptr_t dst, uintptr_t stream) {
            std::vector<uint32_t> flat;
            for (const auto& p : pairs) {
              flat.push_back(p.first);
              flat.push_back(p.second);
            }
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_xcorr(flat.data(), uint32_t(pairs.size()), span, reinterpret_cast<const float*>(scale), L,
                                 reinterpret_cast<int64_t*>(dst), reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_xcorr failed: " + std::to_string(e));
          },
          py::arg("pairs"), py::arg("span"), py::arg("scale_ptr"), py::arg("lags"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue the cross-correlation sums of pairs [(a, b), ..] of series of one ring over the newest min(n, span) rows "
          "after the last refresh: scale [S] floats -> dst [K][2 lags + 1][6] int64 (n, Sx, Sy, Sxy, Sxx, Syy per lag -L .. L).")
      .def(
          "export_joint",
          [](LongWindowSet& w, const std::vector<std::pair<uint32_t, uint32_t>>& pairs, uintptr_t bounds, uint32_t B,
             uintptr_t dst, uintptr_t stream) {
            std::vector<uint32_t> flat;
            for (const auto& p : pairs) {
              flat.push_back(p.first);
              flat.push_back(p.second);
            }
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_joint(flat.data(), uint32_t(pairs.size()), reinterpret_cast<const float*>(bounds), B,
                                 reinterpret_cast<int32_t*>(dst), reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_joint failed: " + std::to_string(e));
          },
          py::arg("pairs"), py::arg("bounds_ptr"), py::arg("num_bounds"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue the joint histograms of pairs [(a, b), ..] of series of one ring after the last refresh: bounds "
          "[S][B] floats -> dst [K][B + 1][B + 1] int32 (rows with bin(x_a) == i and bin(x_b) == j, both valid).")
      .def(
          "export_heatmap",
          [](LongWindowSet& w, uint32_t P, uintptr_t bounds, uint32_t B, uintptr_t dst, uintptr_t stream) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_heatmap(P, reinterpret_cast<const float*>(bounds), B, reinterpret_cast<int32_t*>(dst),
                                   reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_heatmap failed: " + std::to_string(e));
          },
          py::arg("columns"), py::arg("bounds_ptr"), py::arg("num_bounds"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue every series' window heatmap after the last refresh: bounds [S][B] floats -> dst "
          "[S][columns + 1][B + 1] int32 (per-bin counts per slot of window / columns rows).")
      .def(
          "export_excursions",
          [](LongWindowSet& w, uintptr_t thresholds, uint32_t K, uintptr_t dst, uintptr_t work, size_t work_bytes,
             uintptr_t stream) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_excursions(reinterpret_cast<const float*>(thresholds), K, reinterpret_cast<int32_t*>(dst),
                                      reinterpret_cast<void*>(work), work_bytes, reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_excursions failed: " + std::to_string(e));
          },
          py::arg("thresholds_ptr"), py::arg("num_thresholds"), py::arg("dst_ptr"), py::arg("work_ptr"),
          py::arg("work_bytes"), py::arg("stream"),
          "Enqueue every series' window excursions after the last refresh: thresholds [S][K] floats -> dst [S][K][8] "
          "int32 (above, valid, episodes, longest, current, since, leading, rows); work: a caller-owned workspace of "
          "excursion_workspace_bytes(S, K) bytes.")
      .def(
          "export_buckets",
          [](LongWindowSet& w, uintptr_t bounds, uint32_t B, uintptr_t dst, uintptr_t stream) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_buckets(reinterpret_cast<const float*>(bounds), B, reinterpret_cast<double*>(dst),
                                   reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_buckets failed: " + std::to_string(e));
          },
          py::arg("bounds_ptr"), py::arg("num_bounds"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue every series' cumulative le-buckets over the window of the last refresh, streamed from the "
          "device rings: bounds [S][B] floats -> dst [S][B + 1] doubles (samples <= each bound, then the valid count).")
      .def(
          "refresh_node",
          [](LongWindowSet& w, uintptr_t out, uintptr_t stream, float p0, float p1, float p2,
             std::shared_ptr<RcclComm> comm, bool timing, double timeout_s, py::object abandon) {
            std::function<bool()> ab;
            if (!abandon.is_none()) {
              // polled from the host wait with the GIL released: take it for each call
              ab = [abandon]() {
                py::gil_scoped_acquire gil;
                return abandon().cast<bool>();
              };
            }
            py::gil_scoped_release nogil;
            w.refresh_node(reinterpret_cast<float*>(out), reinterpret_cast<void*>(stream), p0, p1, p2, comm.get(),
                           timing, timeout_s, ab);
          },
          py::arg("out_ptr"), py::arg("stream"), py::arg("p0") = 50.0f, py::arg("p1") = 90.0f, py::arg("p2") = 99.0f,
          py::arg("comm") = py::none(), py::arg("timing") = false, py::arg("timeout_s") = 60.0,
          py::arg("abandon") = py::none(),
          "Collective: node-wide statistics over every rank's window (radix select with the digit histograms "
          "all-reduced over `comm` between the passes; None = a one-rank node). out [S][8], last = NaN.")
      .def("set_node_brackets", &LongWindowSet::set_node_brackets, py::arg("series"), py::arg("lo"), py::arg("hi"),
           py::call_guard<py::gil_scoped_release>(),
           "Test hook: the node brackets of one series (3 lo / 3 hi order-preserving keys) for the next node refresh.")
      .def_property_readonly("node_cap", &LongWindowSet::node_cap)
      .def_property_readonly("node_last_maxmid", &LongWindowSet::node_last_maxmid)
      .def("reset_node", &LongWindowSet::reset_node, py::call_guard<py::gil_scoped_release>(),
           "Forget the node's bracket state (every member, at the start of a membership epoch).")
      .def("node_collective_us", &LongWindowSet::node_collective_us,
           "µs of the last timed node refresh's 5 collective steps (synchronises their events).")
      .def("stats", [](const LongWindowSet& w) {
        const auto s = w.stats();
        py::dict d;
        d["refreshes"] = s.refreshes;
        d["node_refreshes"] = s.node_refreshes;
        d["node_resets"] = s.node_resets;
        d["bracket_refreshes"] = s.bracket_refreshes;
        d["passb_chunks"] = s.passb_chunks;
        d["chain_refreshes"] = s.chain_refreshes;
        d["rows_copied"] = s.rows_copied;
        d["bytes_copied"] = s.bytes_copied;
        d["memcpy_calls"] = s.memcpy_calls;
        d["rows_lost"] = s.rows_lost;
        d["graph_launches"] = s.graph_launches;
        d["kernel_launches"] = s.kernel_launches;
        d["ingest_launches"] = s.ingest_launches;  // staging kernels (in place of DMA copies)
        d["fused_refreshes"] = s.fused_refreshes;  // bracket refreshes whose scan B streamed chunks
        d["single_kernel_refreshes"] = s.single_kernel_refreshes;  // ... with no pass B kernel
        d["fused_segments"] = s.fused_segments;
        d["node_record_bytes"] = s.node_record_bytes;  // node bracket records all-gathered (this rank's, summed)
        d["host_stage_ns"] = s.host_stage_ns;  // refresh()'s host time: staging,
        d["host_enqueue_ns"] = s.host_enqueue_ns;  // a bracket refresh's work list + launches,
        d["host_wait_ns"] = s.host_wait_ns;  // and its wait for the report
        return d;
      });

  m.def("set_pinned_host_rings", &set_pinned_host_rings, py::arg("on"));
  m.def("set_pull_mode", &set_pull_mode, py::arg("on"));
  m.def("hip_device_count", &hip_device_count);
  m.def("hip_device_bdf", &hip_device_bdf, py::arg("device"));

  py::class_<DeviceWindowSet, std::shared_ptr<DeviceWindowSet>>(m, "DeviceWindowSet")
      .def(py::init<uint32_t, int>(), py::arg("window"), py::arg("device"))
      .def("add_ring", &DeviceWindowSet::add_ring, py::arg("ring"))
      .def_property_readonly("num_series", &DeviceWindowSet::num_series)
      .def_property_readonly("window", &DeviceWindowSet::window)
      .def_property_readonly("device", &DeviceWindowSet::device)
      .def(
          "refresh",
          [](DeviceWindowSet& w, uintptr_t out, uintptr_t stream, float p0, float p1, float p2, int signal) {
            if (signal < DeviceWindowSet::kSignalNone || signal > DeviceWindowSet::kSignalTagged)
              throw std::invalid_argument("signal: 0 (none), 1 (flag) or 2 (tagged host output)");
            py::gil_scoped_release nogil;
            return w.refresh(reinterpret_cast<float*>(out), reinterpret_cast<void*>(stream), p0, p1, p2, signal);
          },
          py::arg("out_ptr"), py::arg("stream"), py::arg("p0") = 50.f, py::arg("p1") = 90.f, py::arg("p2") = 99.f,
          py::arg("signal") = int(DeviceWindowSet::kSignalFlag),
          "Enqueue the refresh; returns its completion sequence number (0: no completion signal). signal: "
          "0 = none (synchronise the stream), 1 = completion flag, 2 = tagged outputs (out_ptr is host memory, "
          "filled by wait_done()).")
      .def(
          "wait_done",
          [](const DeviceWindowSet& w, uint32_t seq, double timeout_s) {
            py::gil_scoped_release nogil;
            return w.wait_done(seq, timeout_s * 1e6);
          },
          py::arg("seq"), py::arg("timeout_s") = 1.0,
          "Spin until refresh `seq` has written its outputs (flag in mapped host memory); False on timeout, for "
          "an older tagged refresh, or when a newer refresh superseded it (never a mixed copy).")
      .def_property_readonly("superseded", &DeviceWindowSet::superseded)
      .def("invalidate", &DeviceWindowSet::invalidate)
      .def(
          "export_sorted",
          [](const DeviceWindowSet& w, uintptr_t dst, uintptr_t stream) {
            py::gil_scoped_release nogil;
            w.export_sorted(reinterpret_cast<float*>(dst), reinterpret_cast<void*>(stream));
          },
          py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue every series' resident sorted window as [S][1 + W] floats (count, samples, +inf).")
      .def(
          "export_buckets",
          [](const DeviceWindowSet& w, uintptr_t bounds, uint32_t B, uintptr_t dst, uintptr_t stream) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_buckets(reinterpret_cast<const float*>(bounds), B, reinterpret_cast<float*>(dst),
                                   reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_buckets failed: " + std::to_string(e));
          },
          py::arg("bounds_ptr"), py::arg("num_bounds"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue every series' cumulative le-buckets over its resident sorted window: bounds [S][B] -> "
          "dst [S][B + 1] floats (samples <= each bound, then the valid count).")
      .def(
          "export_trend",
          [](const DeviceWindowSet& w, uint32_t P, uintptr_t dst, uintptr_t stream) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_trend(P, reinterpret_cast<float*>(dst), reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_trend failed: " + std::to_string(e));
          },
          py::arg("columns"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue every series' window trend after the last refresh: dst [S][columns + 1][4] floats "
          "(min, max, mean, count per slot of window / columns rows).")
      .def(
          "export_quantiles",
          [](const DeviceWindowSet& w, uint32_t P, uintptr_t dst, uintptr_t stream, float p0, float p1, float p2) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_quantiles(P, p0, p1, p2, reinterpret_cast<float*>(dst), reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_quantiles failed: " + std::to_string(e));
          },
          py::arg("columns"), py::arg("dst_ptr"), py::arg("stream"), py::arg("p0") = 50.0f, py::arg("p1") = 90.0f,
          py::arg("p2") = 99.0f,
          "Enqueue every series' window quantile trend after the last refresh: dst [S][columns + 1][4] floats "
          "(the three percentiles and the count per slot of window / columns rows).")
      .def(
          "export_autocorr",
          [](const DeviceWindowSet& w, uint32_t span, uintptr_t scale, uint32_t L, uintptr_t dst, uintptr_t stream) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_autocorr(span, reinterpret_cast<const float*>(scale), L, reinterpret_cast<int64_t*>(dst),
                                    reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_autocorr failed: " + std::to_string(e));
          },
          py::arg("span"), py::arg("scale_ptr"), py::arg("lags"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue every series' autocorrelation sums over the newest min(n, span) rows after the last refresh: scale "
          "[S] floats -> dst [S][lags + 1][4] int64 (n, Sx, Sy, Sxy per lag).")
      .def(
          "export_periods",
          [](const DeviceWindowSet& w, uint32_t span, uint32_t P, uintptr_t scale, uint32_t L, uintptr_t dst, uintptr_t stream) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_periods(span, P, reinterpret_cast<const float*>(scale), L, reinterpret_cast<int64_t*>(dst),
                                   reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_periods failed: " + std::to_string(e));
          },
          py::arg("span"), py::arg("columns"), py::arg("scale_ptr"), py::arg("lags"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue every series' window period trend after the last refresh: the autocorrelation's sums per trend slot of "
          "the newest min(n, span) rows: scale [S] floats -> dst [S][columns + 1][lags + 1][4] int64.")
      .def(
          "export_xcorr",
          [](const DeviceWindowSet& w, const std::vector<std::pair<uint32_t, uint32_t>>& pairs, uint32_t span, uintptr_t scale,
             uint32_t L, uintptr_t dst, uintptr_t stream) {
            std::vector<uint32_t> flat;
            for (const auto& p : pairs) {
              flat.push_back(p.first);
              flat.push_back(p.second);
            }
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_xcorr(flat.data(), uint32_t(pairs.size()), span, reinterpret_cast<const float*>(scale), L,
                                 reinterpret_cast<int64_t*>(dst), reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_xcorr failed: " + std::to_string(e));
          },
          py::arg("pairs"), py::arg("span"), py::arg("scale_ptr"), py::arg("lags"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue the cross-correlation sums of pairs [(a, b), ..] of series of one ring over the newest min(n, span) rows "
          "after the last refresh: scale [S] floats -> dst [K][2 lags + 1][6] int64 (n, Sx, Sy, Sxy, Sxx, Syy per lag -L .. L).")
      .def(
          "export_joint",
          [](const DeviceWindowSet& w, const std::vector<std::pair<uint32_t, uint32_t>>& pairs, uintptr_t bounds, uint32_t B,
             uintptr_t dst, uintptr_t stream) {
            std::vector<uint32_t> flat;
            for (const auto& p : pairs) {
              flat.push_back(p.first);
              flat.push_back(p.second);
            }
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_joint(flat.data(), uint32_t(pairs.size()), reinterpret_cast<const float*>(bounds), B,
                                 reinterpret_cast<int32_t*>(dst), reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_joint failed: " + std::to_string(e));
          },
          py::arg("pairs"), py::arg("bounds_ptr"), py::arg("num_bounds"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue the joint histograms of pairs [(a, b), ..] of series of one ring after the last refresh: bounds "
          "[S][B] floats -> dst [K][B + 1][B + 1] int32 (rows with bin(x_a) == i and bin(x_b) == j, both valid).")
      .def(
          "export_heatmap",
          [](const DeviceWindowSet& w, uint32_t P, uintptr_t bounds, uint32_t B, uintptr_t dst, uintptr_t stream) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_heatmap(P, reinterpret_cast<const float*>(bounds), B, reinterpret_cast<int32_t*>(dst),
                                   reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_heatmap failed: " + std::to_string(e));
          },
          py::arg("columns"), py::arg("bounds_ptr"), py::arg("num_bounds"), py::arg("dst_ptr"), py::arg("stream"),
          "Enqueue every series' window heatmap after the last refresh: bounds [S][B] floats -> dst "
          "[S][columns + 1][B + 1] int32 (per-bin counts per slot of window / columns rows).")
      .def(
          "export_excursions",
          [](const DeviceWindowSet& w, uintptr_t thresholds, uint32_t K, uintptr_t dst, uintptr_t work, size_t work_bytes,
             uintptr_t stream) {
            int e;
            {
              py::gil_scoped_release nogil;
              e = w.export_excursions(reinterpret_cast<const float*>(thresholds), K, reinterpret_cast<int32_t*>(dst),
                                      reinterpret_cast<void*>(work), work_bytes, reinterpret_cast<void*>(stream));
            }
            if (e != 0) throw std::runtime_error("export_excursions failed: " + std::to_string(e));
          },
          py::arg("thresholds_ptr"), py::arg("num_thresholds"), py::arg("dst_ptr"), py::arg("work_ptr"),
          py::arg("work_bytes"), py::arg("stream"),
          "Enqueue every series' window excursions after the last refresh: thresholds [S][K] floats -> dst [S][K][8] "
          "int32 (above, valid, episodes, longest, current, since, leading, rows); work: a caller-owned workspace of "
          "excursion_workspace_bytes(S, K) bytes.")
      .def("stats", [](const DeviceWindowSet& w) {
        auto st = w.stats();
        py::dict d;
        d["refreshes"] = st.refreshes;
        d["rows_copied"] = st.rows_copied;
        d["bytes_copied"] = st.bytes_copied;
        d["memcpy_calls"] = st.memcpy_calls;
        d["launches"] = st.launches;
        d["incremental_launches"] = st.incremental_launches;
        d["pulled_series"] = st.pulled_series;
        d["inline_rows"] = st.inline_rows;
        return d;
      });

  // Direct, stateless kernel entry for tests/benchmarks: one device ring
  // [mask + 1][stride] float32 (time-major), window rows head - n .. head - 1, one
  // output row of 8 statistics per listed column.
  m.def(
      "window_stats_raw",
      [](uintptr_t base, uint64_t head, uint32_t stride, uint32_t mask, uint32_t n, const std::vector<uint32_t>& cols,
         uintptr_t out, uintptr_t stream, float p0, float p1, float p2) {
        if (cols.empty()) return;
        if (cols.size() > size_t(kMaxSeriesPerLaunch)) throw std::invalid_argument("too many series for one launch");
        if (n > mask + 1 || n > head) throw std::invalid_argument("n must be <= capacity and <= head");
        if (((mask + 1) & mask) != 0) throw std::invalid_argument("capacity must be a power of two");
        if (n > 32768) throw std::invalid_argument("window must be <= 32768");
        StatsArgs args{};
        args.pct[0] = p0;
        args.pct[1] = p1;
        args.pct[2] = p2;
        args.num_rings = 1;
        RingHead& r = args.rings[0].h;
        for (size_t j = 0; j < cols.size(); ++j) {
          if (cols[j] >= stride) throw std::invalid_argument("column must be < stride");
          if (cols[j] != cols[0] + j) throw std::invalid_argument("columns must be one ascending run");
        }
        // the run of columns c0 .. c0 + count - 1 as a ring that starts at column c0
        r.base = reinterpret_cast<float*>(base) + cols[0];  // read only: no state, nothing entering
        r.head = head;
        r.pred_head0 = ~0ull;
        r.stride = stride;
        r.cols = uint32_t(cols.size());
        r.mask = mask;
        r.n = n;
        args.num_series = uint32_t(cols.size());
        int e;
        {
          py::gil_scoped_release nogil;
          e = launch_window_stats(args, sort_width_for(std::max<uint32_t>(n, 1)), reinterpret_cast<float*>(out),
                                  reinterpret_cast<void*>(stream));
        }
        if (e != 0) throw std::runtime_error("window_stats launch failed: " + std::to_string(e));
      },
      py::arg("base_ptr"), py::arg("head"), py::arg("stride"), py::arg("mask"), py::arg("n"), py::arg("cols"),
      py::arg("out_ptr"), py::arg("stream"), py::arg("p0") = 50.f, py::arg("p1") = 90.f, py::arg("p2") = 99.f);
  m.def("sort_width_for", &sort_width_for, py::arg("n"));
  // for the CPU tests only (tests/test_window_stats_rules.py): the rules the window-stats kernel
  // and DeviceWindowSet run (window_stats_rules.h); not an interface of the service
  m.attr("MAX_INCREMENTAL") = int(kMaxIncremental);
  m.def("ws_incremental_step", [](uint64_t h0, uint32_t n0, uint32_t cur, uint64_t h1, uint32_t n1, uint64_t depth,
                                  uint32_t sorted_cap) {
    const IncStep s = incremental_step(h0, n0, cur, h1, n1, depth, sorted_cap);
    return py::make_tuple(s.ok, s.kadd, s.krem);
  });
  m.def("ws_next_half", &next_half, py::arg("incremental"), py::arg("have_state"), py::arg("cur"));
  m.def("ws_changed_span", [](uint32_t kr, uint32_t ka, uint32_t first_leave, uint32_t last_leave, uint32_t first_ins,
                              uint32_t last_ins, uint32_t nv) {
    const Span s = changed_span(kr, ka, first_leave, last_leave, first_ins, last_ins, nv);
    return py::make_tuple(s.lo, s.hi);
  });
  m.def("ws_one_row_map", [](uint32_t kr, uint32_t ka, uint32_t leave, uint32_t ins) {
    const OneRowMap m = one_row_map(kr, ka, leave, ins);
    return py::make_tuple(m.x, m.pn);
  });
  m.def("ws_one_row_src", [](uint32_t x, uint32_t pn, uint32_t p) { return OneRowMap{x, pn}.src(p); });
  m.def("ws_wanted_positions", [](uint32_t nv, std::array<float, 3> pct) {
    const double qfrac[3] = {double(pct[0]) / 100.0, double(pct[1]) / 100.0, double(pct[2]) / 100.0};
    uint32_t idx[8];
    float frac[3];
    wanted_positions(nv, qfrac, idx, frac);
    return py::make_tuple(std::vector<uint32_t>(idx, idx + 8), std::vector<float>(frac, frac + 3));
  });
  m.def("ws_percentile_between", &percentile_between, py::arg("x0"), py::arg("x1"), py::arg("frac"));
  m.attr("WS_INLINE_ROWS") = kInlineRows;  // most entering rows per ring sent in the kernel argument
  m.def("ws_launch_shape", [](uint32_t pad_pow2, bool incremental, uint32_t max_new_rows, uint32_t small_k) {
    const LaunchShape s = launch_shape(pad_pow2, incremental, max_new_rows, small_k);
    return py::make_tuple(s.nt, s.e);
  });
  m.def("rccl_load", &rccl_load, py::arg("lib_path") = "",
        "Load RCCL without creating anything; returns its version code (every rank, before the init).");
  m.def(
      "rccl_unique_id", [](const std::string& lib) { return py::bytes(rccl_unique_id(lib)); }, py::arg("lib_path") = "",
      "A new RCCL communicator's 128-byte unique id (rank 0; share it with every rank).");
  py::class_<RcclComm, std::shared_ptr<RcclComm>>(m, "RcclComm")
      .def(py::init([](int device, int nranks, int rank, py::bytes uid, const std::string& lib, double timeout_s) {
             std::string id = uid;
             py::gil_scoped_release nogil;  // collective: waits (at most timeout_s) until every rank joins
             return std::make_shared<RcclComm>(device, nranks, rank, id, lib, timeout_s);
           }),
           py::arg("device"), py::arg("nranks"), py::arg("rank"), py::arg("unique_id"), py::arg("lib_path") = "",
           py::arg("timeout_s") = 120.0)
      .def(
          "all_gather",
          [](RcclComm& c, uintptr_t send, uintptr_t recv, size_t count, uintptr_t stream) {
            c.all_gather(reinterpret_cast<const float*>(send), reinterpret_cast<float*>(recv), count,
                         reinterpret_cast<void*>(stream));
          },
          py::arg("send_ptr"), py::arg("recv_ptr"), py::arg("count"), py::arg("stream"),
          "Enqueue ncclAllGather of `count` float32 per rank on `stream`.")
      .def(
          "all_gather_bytes",
          [](RcclComm& c, uintptr_t send, uintptr_t recv, size_t bytes, uintptr_t stream) {
            c.all_gather_bytes(reinterpret_cast<const void*>(send), reinterpret_cast<void*>(recv), bytes,
                               reinterpret_cast<void*>(stream));
          },
          py::arg("send_ptr"), py::arg("recv_ptr"), py::arg("bytes"), py::arg("stream"),
          "Enqueue ncclAllGather of `bytes` per rank on `stream` (moved bit for bit).")
      .def(
          "all_reduce_sum_u32",
          [](RcclComm& c, uintptr_t send, uintptr_t recv, size_t count, uintptr_t stream) {
            c.all_reduce_sum_u32(reinterpret_cast<const uint32_t*>(send), reinterpret_cast<uint32_t*>(recv), count,
                                 reinterpret_cast<void*>(stream));
          },
          py::arg("send_ptr"), py::arg("recv_ptr"), py::arg("count"), py::arg("stream"),
          "Enqueue ncclAllReduce(sum) of `count` uint32 on `stream`.")
      .def(
          "view",
          [](const RcclComm& c) {
            const RcclView v = c.view();
            py::dict d;
            d["nranks"] = v.nranks;
            d["rank"] = v.rank;
            d["device"] = v.device;
            return d;
          },
          "RCCL's own view: ncclCommCount, ncclCommUserRank, ncclCommCuDevice (-1 where refused).")
      .def("async_error", &RcclComm::async_error, "0 while healthy, else the communicator's ncclResult_t")
      .def("abort", &RcclComm::abort, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("init_seconds", &RcclComm::init_seconds)
      .def_property_readonly("nranks", &RcclComm::nranks)
      .def_property_readonly("rank", &RcclComm::rank);
  py::class_<HostPublisher, std::shared_ptr<HostPublisher>>(m, "HostPublisher")
      .def(py::init<int, bool>(), py::arg("device"), py::arg("tagged") = true)
      .def(
          "publish",
          [](HostPublisher& p, uintptr_t src, uintptr_t dst, uint32_t n, uintptr_t stream) {
            return p.publish(reinterpret_cast<const float*>(src), reinterpret_cast<float*>(dst), n,
                             reinterpret_cast<void*>(stream));
          },
          py::arg("src_ptr"), py::arg("dst_ptr"), py::arg("n"), py::arg("stream"),
          "Enqueue: copy n floats device -> pinned host, then publish; returns the sequence number.")
      .def(
          "wait",
          [](const HostPublisher& p, uint32_t seq, double timeout_s) {
            py::gil_scoped_release nogil;
            return p.wait(seq, timeout_s * 1e6);
          },
          py::arg("seq"), py::arg("timeout_s") = 1.0)
      .def_property_readonly("superseded", &HostPublisher::superseded,
                             "Tagged waits that found a newer publication in the words (no mixed copy returned).");
  m.def(
      "spin",
      [](uint32_t workgroups, double us, uintptr_t stream) {
        const int e = launch_spin(workgroups, us, reinterpret_cast<void*>(stream));
        if (e != 0) throw std::runtime_error("spin launch failed: " + std::to_string(e));
      },
      py::arg("workgroups"), py::arg("us"), py::arg("stream"),
      "Calibration load: `workgroups` one-wave workgroups, each busy for `us` microseconds.");
  m.def(
      "calib_gather32",
      [](uintptr_t src, uint64_t src_bytes, uintptr_t out, uint64_t out_bytes, uint32_t threads, uint32_t seed,
         uintptr_t stream) {
        const int e = launch_gather32(reinterpret_cast<const void*>(src), src_bytes, reinterpret_cast<void*>(out),
                                      out_bytes, threads, seed, reinterpret_cast<void*>(stream));
        if (e != 0) throw std::runtime_error("gather32 launch failed: " + std::to_string(e));
      },
      py::arg("src"), py::arg("src_bytes"), py::arg("out"), py::arg("out_bytes"), py::arg("threads"),
      py::arg("seed"), py::arg("stream"), "Calibration load: one 32 B read per thread at a random 32 B slot.");
  m.def(
      "calib_store64",
      [](uintptr_t dst, uint64_t dst_bytes, uint32_t threads, uintptr_t stream) {
        const int e = launch_store64(reinterpret_cast<void*>(dst), dst_bytes, threads, reinterpret_cast<void*>(stream));
        if (e != 0) throw std::runtime_error("store64 launch failed: " + std::to_string(e));
      },
      py::arg("dst"), py::arg("dst_bytes"), py::arg("threads"), py::arg("stream"),
      "Calibration load: one 64 B store per thread, 256 B apart.");
  m.def(
      "calib_store32",
      [](uintptr_t dst, uint64_t dst_bytes, uint32_t threads, uintptr_t stream) {
        const int e = launch_store32(reinterpret_cast<void*>(dst), dst_bytes, threads, reinterpret_cast<void*>(stream));
        if (e != 0) throw std::runtime_error("store32 launch failed: " + std::to_string(e));
      },
      py::arg("dst"), py::arg("dst_bytes"), py::arg("threads"), py::arg("stream"),
      "Calibration load: one 32 B store per thread, 256 B apart.");
  m.def(
      "node_select",
      [](uintptr_t node, uint32_t N, uint32_t S, uint32_t W, uintptr_t out, uintptr_t stream, float p0, float p1,
         float p2) {
        int e;
        {
          py::gil_scoped_release nogil;
          e = launch_node_select(reinterpret_cast<const float*>(node), N, S, W, p0, p1, p2, reinterpret_cast<float*>(out),
                                 reinterpret_cast<void*>(stream));
        }
        if (e != 0) throw std::runtime_error("node_select launch failed: " + std::to_string(e));
      },
      py::arg("node_ptr"), py::arg("n_ranks"), py::arg("num_series"), py::arg("window"), py::arg("out_ptr"),
      py::arg("stream"), py::arg("p0") = 50.f, py::arg("p1") = 90.f, py::arg("p2") = 99.f,
      "Order statistics over the union of N ranks' exported sorted windows: node [N][S][1 + W] -> out [S][8].");
  m.attr("MAX_BUCKETS") = int(kMaxBuckets);
  m.attr("BUCKET_SERIES_PER_LAUNCH") = int(kBucketSeriesPerLaunch);
  m.def(
      "bucket_blocks",
      [](uintptr_t blocks, uint32_t N, uint32_t S, uint32_t W, uintptr_t bounds, uint32_t B, uintptr_t per_rank,
         uintptr_t node, uintptr_t stream) {
        int e;
        {
          py::gil_scoped_release nogil;
          e = launch_bucket_blocks(reinterpret_cast<const float*>(blocks), N, S, W,
                                   reinterpret_cast<const float*>(bounds), B, reinterpret_cast<float*>(per_rank),
                                   reinterpret_cast<float*>(node), reinterpret_cast<void*>(stream));
        }
        if (e != 0) throw std::runtime_error("bucket_blocks failed: " + std::to_string(e));
      },
      py::arg("blocks_ptr"), py::arg("n_ranks"), py::arg("num_series"), py::arg("window"), py::arg("bounds_ptr"),
      py::arg("num_bounds"), py::arg("per_rank_ptr"), py::arg("node_ptr"), py::arg("stream"),
      "Cumulative le-buckets over export blocks [N][S][1 + W] and bounds [S][B]: per_rank [N][S][B + 1] and / or "
      "node [S][B + 1] (the sum over the ranks); a pointer of 0 skips that output.");
  m.def(
      "bucket_ring",
      [](uintptr_t base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n, uintptr_t bounds,
         uint32_t B, uintptr_t dst, uintptr_t stream) {
        int e;
        {
          py::gil_scoped_release nogil;
          e = launch_bucket_ring(reinterpret_cast<const float*>(base), stride, cols, depth, head, n,
                                 reinterpret_cast<const float*>(bounds), B, reinterpret_cast<double*>(dst),
                                 reinterpret_cast<void*>(stream));
        }
        if (e != 0) throw std::runtime_error("bucket_ring failed: " + std::to_string(e));
      },
      py::arg("base_ptr"), py::arg("stride"), py::arg("cols"), py::arg("depth"), py::arg("head"), py::arg("n"),
      py::arg("bounds_ptr"), py::arg("num_bounds"), py::arg("dst_ptr"), py::arg("stream"),
      "Cumulative le-buckets of one time-major ring [depth][stride] (row r at slot r & (depth - 1)) whose window is "
      "rows [head - n, head): bounds [cols][B] floats -> dst [cols][B + 1] doubles.");
  m.attr("MAX_EXCURSION_THRESHOLDS") = int(kMaxExcursionThresholds);
  m.attr("MAX_EXCURSION_CHUNKS") = int(kMaxExcursionChunks);
  m.def("excursion_workspace_bytes", &excursion_workspace_bytes, py::arg("series"), py::arg("num_thresholds"),
        "Bytes of the caller-owned workspace of the excursion exports for `series` series (a ring's stride, or every "
        "series of a set) and K thresholds; 0 for a K outside [1, 4].");
  m.def("excursion_plan_chunk_rows", &excursion_plan_chunk_rows, py::arg("n"),
        "Rows per chunk the excursion stream plans for a window of n rows.");
  m.def("excursion_chunk_count", &excursion_chunk_count, py::arg("depth"), py::arg("head"), py::arg("n"),
        py::arg("chunk_rows"), "Chunks of the window [head - n, head) of a ring of depth rows cut every chunk_rows rows.");
  m.def(
      "excursion_ring",
      [](uintptr_t base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n, uintptr_t thresholds,
         uint32_t K, uint32_t chunk_rows, uintptr_t dst, uintptr_t work, size_t work_bytes, uintptr_t stream) {
        int e;
        {
          py::gil_scoped_release nogil;
          e = launch_excursion_ring(reinterpret_cast<const float*>(base), stride, cols, depth, head, n,
                                    reinterpret_cast<const float*>(thresholds), K, chunk_rows,
                                    reinterpret_cast<int32_t*>(dst), reinterpret_cast<void*>(work), work_bytes,
                                    reinterpret_cast<void*>(stream));
        }
        if (e != 0) throw std::runtime_error("excursion_ring failed: " + std::to_string(e));
      },
      py::arg("base_ptr"), py::arg("stride"), py::arg("cols"), py::arg("depth"), py::arg("head"), py::arg("n"),
      py::arg("thresholds_ptr"), py::arg("num_thresholds"), py::arg("chunk_rows"), py::arg("dst_ptr"), py::arg("work_ptr"),
      py::arg("work_bytes"), py::arg("stream"),
      "Window excursions of one time-major ring [depth][stride] (row r at slot r & (depth - 1)) whose window is rows "
      "[head - n, head): thresholds [cols][K] floats -> dst [cols][K][8] int32. chunk_rows 0 plans the chunks.");
  m.attr("MAX_TREND_COLUMNS") = int(kMaxTrendColumns);
  m.attr("MAX_TREND_ROWS_PER_COLUMN") = int(kMaxTrendRowsPerColumn);
  m.def(
      "trend_ring",
      [](uintptr_t base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n, uint32_t P,
         uint32_t rows_per_col, uintptr_t dst, uintptr_t stream) {
        int e;
        {
          py::gil_scoped_release nogil;
          e = launch_trend_ring(reinterpret_cast<const float*>(base), stride, cols, depth, head, n, P, rows_per_col,
                                reinterpret_cast<float*>(dst), reinterpret_cast<void*>(stream));
        }
        if (e != 0) throw std::runtime_error("trend_ring failed: " + std::to_string(e));
      },
      py::arg("base_ptr"), py::arg("stride"), py::arg("cols"), py::arg("depth"), py::arg("head"), py::arg("n"),
      py::arg("columns"), py::arg("rows_per_col"), py::arg("dst_ptr"), py::arg("stream"),
      "Window trend of one time-major ring [depth][stride] (row r at slot r & (depth - 1)) whose window is rows "
      "[head - n, head): dst [cols][columns + 1][4] floats (min, max, mean, count per slot of rows_per_col rows).");
  m.attr("QUANTILE_SORT_MAX_ROWS") = int(kQuantileSortMaxRows);  // rows per column: above, the radix select
  m.def(
      "quantile_ring",
      [](uintptr_t base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n, uint32_t P,
         uint32_t rows_per_col, uintptr_t dst, uintptr_t stream, float p0, float p1, float p2) {
        int e;
        {
          py::gil_scoped_release nogil;
          e = launch_quantile_ring(reinterpret_cast<const float*>(base), stride, cols, depth, head, n, P, rows_per_col, p0,
                                   p1, p2, reinterpret_cast<float*>(dst), reinterpret_cast<void*>(stream));
        }
        if (e != 0) throw std::runtime_error("quantile_ring failed: " + std::to_string(e));
      },
      py::arg("base_ptr"), py::arg("stride"), py::arg("cols"), py::arg("depth"), py::arg("head"), py::arg("n"),
      py::arg("columns"), py::arg("rows_per_col"), py::arg("dst_ptr"), py::arg("stream"), py::arg("p0") = 50.0f,
      py::arg("p1") = 90.0f, py::arg("p2") = 99.0f,
      "Window quantile trend of one time-major ring [depth][stride] (row r at slot r & (depth - 1)) whose window is "
      "rows [head - n, head): dst [cols][columns + 1][4] floats (three percentiles and the count per slot).");
  m.def(
      "heatmap_ring",
      [](uintptr_t base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n, uint32_t P,
         uint32_t rows_per_col, uintptr_t bounds, uint32_t B, uintptr_t dst, uintptr_t stream) {
        int e;
        {
          py::gil_scoped_release nogil;
          e = launch_heatmap_ring(reinterpret_cast<const float*>(base), stride, cols, depth, head, n, P, rows_per_col,
                                  reinterpret_cast<const float*>(bounds), B, reinterpret_cast<int32_t*>(dst),
                                  reinterpret_cast<void*>(stream));
        }
        if (e != 0) throw std::runtime_error("heatmap_ring failed: " + std::to_string(e));
      },
      py::arg("base_ptr"), py::arg("stride"), py::arg("cols"), py::arg("depth"), py::arg("head"), py::arg("n"),
      py::arg("columns"), py::arg("rows_per_col"), py::arg("bounds_ptr"), py::arg("num_bounds"), py::arg("dst_ptr"),
      py::arg("stream"),
      "Window heatmap of one time-major ring [depth][stride] (row r at slot r & (depth - 1)) whose window is rows "
      "[head - n, head): bounds [cols][B] floats -> dst [cols][columns + 1][B + 1] int32 (per-bin counts per slot).");
  m.def(
      "periods_ring",
      [](uintptr_t base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n, uint32_t span, uint32_t P,
         uintptr_t scale, uint32_t L, uintptr_t dst, uint32_t split, uintptr_t stream) {
        int e;
        {
          py::gil_scoped_release nogil;
          e = launch_periods_ring(reinterpret_cast<const float*>(base), stride, cols, depth, head, n, span, P,
                                  reinterpret_cast<const float*>(scale), L, reinterpret_cast<int64_t*>(dst), split,
                                  reinterpret_cast<void*>(stream));
        }
        if (e != 0) throw std::runtime_error("periods_ring failed: " + std::to_string(e));
      },
      py::arg("base_ptr"), py::arg("stride"), py::arg("cols"), py::arg("depth"), py::arg("head"), py::arg("n"),
      py::arg("span"), py::arg("columns"), py::arg("scale_ptr"), py::arg("lags"), py::arg("dst_ptr"), py::arg("split"),
      py::arg("stream"),
      "Window period trend of every column of one time-major ring [depth][stride] (row r at slot r & (depth - 1)): the "
      "autocorrelation's sums per trend slot of the newest min(n, span) rows of the window [head - n, head): scale [cols] "
      "floats -> dst [cols][columns + 1][lags + 1][4] int64. split 0: the plan decides; else workgroups per slot.");
  m.def(
      "autocorr_ring",
      [](uintptr_t base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n, uint32_t span,
         uintptr_t scale, uint32_t L, uintptr_t dst, uintptr_t stream, uint32_t share) {
        int e;
        {
          py::gil_scoped_release nogil;
          e = launch_autocorr_ring(reinterpret_cast<const float*>(base), stride, cols, depth, head, n, span,
                                   reinterpret_cast<const float*>(scale), L, reinterpret_cast<int64_t*>(dst),
                                   reinterpret_cast<void*>(stream), share);
        }
        if (e != 0) throw std::runtime_error("autocorr_ring failed: " + std::to_string(e));
      },
      py::arg("base_ptr"), py::arg("stride"), py::arg("cols"), py::arg("depth"), py::arg("head"), py::arg("n"),
      py::arg("span"), py::arg("scale_ptr"), py::arg("lags"), py::arg("dst_ptr"), py::arg("stream"), py::arg("share") = 0,
      "Autocorrelation sums of every column of one time-major ring [depth][stride] (row r at slot r & (depth - 1)) over "
      "the newest min(n, span) rows of the window [head - n, head): scale [cols] floats -> dst [cols][lags + 1][4] int64. "
      "share 0: the launch rule decides; else chunks of 1024 rows per workgroup.");
  m.def(
      "xcorr_ring",
      [](uintptr_t base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n, uint32_t span,
         uintptr_t scale, const std::vector<std::pair<uint32_t, uint32_t>>& pairs, uint32_t L, uintptr_t dst, uintptr_t stream,
         uint32_t share) {
        std::vector<uint32_t> flat;
        for (const auto& p : pairs) {
          flat.push_back(p.first);
          flat.push_back(p.second);
        }
        int e;
        {
          py::gil_scoped_release nogil;
          e = launch_xcorr_ring(reinterpret_cast<const float*>(base), stride, cols, depth, head, n, span,
                                reinterpret_cast<const float*>(scale), flat.data(), uint32_t(pairs.size()), L,
                                reinterpret_cast<int64_t*>(dst), reinterpret_cast<void*>(stream), share);
        }
        if (e != 0) throw std::runtime_error("xcorr_ring failed: " + std::to_string(e));
      },
      py::arg("base_ptr"), py::arg("stride"), py::arg("cols"), py::arg("depth"), py::arg("head"), py::arg("n"),
      py::arg("span"), py::arg("scale_ptr"), py::arg("pairs"), py::arg("lags"), py::arg("dst_ptr"), py::arg("stream"),
      py::arg("share") = 0,
      "Cross-correlation sums of pairs [(a, b), ..] of columns of one time-major ring [depth][stride] (row r at slot r & (depth - 1)) "
      "over the newest min(n, span) rows of the window [head - n, head): scale [cols] floats -> dst [K][2 lags + 1][6] int64. "
      "share 0: the launch rule decides; else chunks of 1024 rows per workgroup.");
  m.def(
      "joint_ring",
      [](uintptr_t base, uint32_t stride, uint32_t cols, uint32_t depth, uint64_t head, uint32_t n,
         const std::vector<std::pair<uint32_t, uint32_t>>& pairs, uintptr_t bounds, uint32_t B, uintptr_t dst,
         uintptr_t stream) {
        std::vector<uint32_t> flat;
        for (const auto& p : pairs) {
          flat.push_back(p.first);
          flat.push_back(p.second);
        }
        int e;
        {
          py::gil_scoped_release nogil;
          e = launch_joint_ring(reinterpret_cast<const float*>(base), stride, cols, depth, head, n, flat.data(),
                                uint32_t(pairs.size()), reinterpret_cast<const float*>(bounds), B,
                                reinterpret_cast<int32_t*>(dst), reinterpret_cast<void*>(stream));
        }
        if (e != 0) throw std::runtime_error("joint_ring failed: " + std::to_string(e));
      },
      py::arg("base_ptr"), py::arg("stride"), py::arg("cols"), py::arg("depth"), py::arg("head"), py::arg("n"),
      py::arg("pairs"), py::arg("bounds_ptr"), py::arg("num_bounds"), py::arg("dst_ptr"), py::arg("stream"),
      "Joint histograms of pairs [(a, b), ..] of columns of one time-major ring [depth][stride] (row r at slot r & "
      "(depth - 1)) whose window is rows [head - n, head): bounds [cols][B] floats -> dst [K][B + 1][B + 1] int32.");

  // ---- native frame renderer (csrc/frame_render.h) ---------------------------------
  py::class_<FramePlan, std::shared_ptr<FramePlan>>(m, "FramePlan")
      .def(py::init([](py::list panels, std::vector<int> sel_rows, int power_col, std::string headers_json,
                       std::string stats_columns_json, int num_columns, bool window, std::string window_gpus_json,
                       std::string window_series_json, std::string window_stats_json, std::vector<int> window_stat_idx,
                       int window_series) {
             auto p = std::make_shared<FramePlan>();
             for (auto item : panels) {
               auto t = item.cast<py::tuple>();
               if (t.size() != 8) throw std::invalid_argument("panel = (key_prefix, head, mid, tail, max_val, src, row, col)");
               PanelPlan pp;
               pp.key_prefix = t[0].cast<std::string>();
               pp.head = t[1].cast<std::string>();
               pp.mid = t[2].cast<std::string>();
               pp.tail = t[3].cast<std::string>();
               pp.max_val = t[4].cast<double>();
               pp.src = t[5].cast<int>();
               pp.row = t[6].cast<int>();
               pp.col = t[7].cast<int>();
               if (pp.src < 0 || pp.src > 2 || pp.col < 0 || (pp.src != 2 && pp.col >= num_columns))
                 throw std::invalid_argument("panel column out of range");
               p->panels.push_back(std::move(pp));
             }
             p->sel_rows = std::move(sel_rows);
             p->power_col = power_col;
             p->headers_json = std::move(headers_json);
             p->stats_columns_json = std::move(stats_columns_json);
             p->num_columns = num_columns;
             p->window = window;
             p->window_gpus_json = std::move(window_gpus_json);
             p->window_series_json = std::move(window_series_json);
             p->window_stats_json = std::move(window_stats_json);
             p->window_stat_idx = std::move(window_stat_idx);
             p->window_series = window_series;
             return p;
           }),
           py::arg("panels"), py::arg("sel_rows"), py::arg("power_col"), py::arg("headers_json"),
           py::arg("stats_columns_json"), py::arg("num_columns"), py::arg("window"), py::arg("window_gpus_json"),
           py::arg("window_series_json"), py::arg("window_stats_json"), py::arg("window_stat_idx"),
           py::arg("window_series"));
  m.def(
      "render_frame",
      [](const FramePlan& plan, py::array_t<double, py::array::c_style | py::array::forcecast> values, py::object window,
         const std::string& ts_key, const std::string& updated_json, bool as_bytes) -> py::object {
        if (values.ndim() != 2 || values.shape(1) != plan.num_columns) throw std::invalid_argument("values must be [G, C]");
        const int G = int(values.shape(0));
        for (const auto& p : plan.panels)
          if (p.src == 0 && p.row >= G) throw std::invalid_argument("panel row out of range");
        for (int r : plan.sel_rows)
          if (r < 0 || r >= G) throw std::invalid_argument("selected row out of range");
        py::array_t<float, py::array::c_style | py::array::forcecast> w;
        const float* wp = nullptr;
        if (plan.window && !window.is_none()) {
          w = window.cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
          if (w.ndim() != 3 || w.shape(0) != G || w.shape(1) != plan.window_series || w.shape(2) != 8)
            throw std::invalid_argument("window must be [G, S, 8]");
          wp = w.data();
        }
        thread_local std::string s;  // capacity kept across refreshes: no page faults per frame
        {
          py::gil_scoped_release nogil;  // renders beside Python threads
          render_frame_into(s, plan, values.data(), G, wp, ts_key, updated_json);
        }
        if (as_bytes) return py::bytes(s.data(), s.size());  // what a socket / file writer takes
        if (plan.all_ascii() && is_ascii(ts_key) && is_ascii(updated_json)) {
          // every byte is 7-bit (templates checked once, numbers are ASCII): build the
          // str by copy instead of a UTF-8 decode of the whole payload
          PyObject* o = PyUnicode_New(py::ssize_t(s.size()), 127);
          if (!o) throw py::error_already_set();
          std::memcpy(PyUnicode_1BYTE_DATA(o), s.data(), s.size());
          return py::reinterpret_steal<py::str>(o);
        }
        return py::str(s);
      },
      py::arg("plan"), py::arg("values"), py::arg("window"), py::arg("ts_key"), py::arg("updated_json"),
      py::arg("as_bytes") = false);
  m.def("py_round2_repr", [](double x) {
    std::string s;
    append_round2(s, x);
    return s;
  });
  m.def("py_float_repr", [](double x) {
    std::string s;
    append_py_float(s, x);
    return s;
  });
}
