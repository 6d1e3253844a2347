// Scripted stand-in for libamd_smi.so, built by tests/test_energy_trace.py into a temporary directory and found
// by the sampler's dlopen("libamd_smi.so") through LD_LIBRARY_PATH of a child process.  No GPU is touched.
//
// The energy accumulator of GPU g is a pure function of CLOCK_MONOTONIC:
//
//   tq  = origin + floor((now - origin) / cadence) * cadence          (the last firmware update)
//   acc = base + floor(E_g(tq) / res) - back_g(tq)                    (counts)
//   ts  = tq - ts_offset                                              (FAKE_SMI_TS_MODE=ns)
//
// E_g(t) is the integral from `origin` to t of a piecewise-constant power schedule with integer watts and
// integer-nanosecond break points, so it is an integer number of nanojoules; `res` is the float 15.259 uJ, an
// exact binary fraction, and the division is done in 128-bit integers.  The test holds the same E_g in Python
// integers: that is its reference.
//
// Environment (times in ns; *_<g> per GPU index g; schedule and event times are relative to the origin):
//   FAKE_SMI_ORIGIN_NS      absolute CLOCK_MONOTONIC origin of the grid and of every schedule (required)
//   FAKE_SMI_NGPU           number of GPUs (1)
//   FAKE_SMI_CPU_BETWEEN    1: a processor handle of CPU type is listed after GPU 0
//   FAKE_SMI_CADENCE_NS     update cadence (16000000)
//   FAKE_SMI_POWER_<g>      "W0,t1:W1,t2:W2,...": W0 up to t1, W1 from t1, ... (300)
//   FAKE_SMI_TS_MODE        ns | zero | ticks10 (timestamp in 10 ns ticks)
//   FAKE_SMI_TS_OFFSET_NS   device clock = host clock - offset (123456789012)
//   FAKE_SMI_ACC_BASE       accumulator value at the origin (1000000007)
//   FAKE_SMI_FAIL_<g>       "a:b": energy reads fail for a <= now - origin < b; "always"
//   FAKE_SMI_BLOCK          "t:dur:after|before": the first energy read with now - origin >= t sleeps dur ns,
//                           after it has taken its reading (the caller sees it late) or before
//   FAKE_SMI_BACK_<g>       "t:counts": from the update at t on the accumulator is `counts` lower
//   FAKE_SMI_CURPOWER_<g>, FAKE_SMI_SOCKPOWER_<g>, FAKE_SMI_GFX_<g>, FAKE_SMI_UMC_<g>   uint32 / uint64 fields
//   FAKE_SMI_VRAM_<g>       "used:total" in MB
#include <amd_smi/amdsmi.h>
#include <time.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace {

struct Proc {
  processor_type_t type;
  int gpu;
};

struct Gpu {
  std::vector<std::pair<int64_t, int64_t>> sched;  // (start relative to origin, watts); first start = 0
  bool fail_always = false;
  int64_t fail_a = 0, fail_b = 0;
  int64_t back_t = INT64_MAX, back_counts = 0;
  uint32_t cur_power = 0, gfx = 0, umc = 0, vram_used = 0, vram_total = 0;
  uint64_t sock_power = 0;
  bool have_cur = false;
};

struct State {
  bool ready = false;
  int64_t origin = 0, cadence = 16000000, ts_offset = 123456789012ll;
  uint64_t base = 1000000007ull;
  int ts_mode = 0;  // 0 ns, 1 zero, 2 ticks10
  float res = 15.259f;
  int64_t res_m = 0;  // res = res_m * 2^-res_s uJ
  int res_s = 0;
  int64_t block_t = INT64_MAX, block_dur = 0;
  bool block_after = true;
  std::atomic<bool> blocked{false};
  std::vector<Gpu> gpus;
  std::vector<Proc> procs;
} S;

int64_t now_ns() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return int64_t(ts.tv_sec) * 1000000000ll + int64_t(ts.tv_nsec);
}

std::string envg(const char* name, int g) {
  std::string k = std::string("FAKE_SMI_") + name;
  if (g >= 0) k += "_" + std::to_string(g);
  const char* v = getenv(k.c_str());
  return v ? v : "";
}

int64_t env_i64(const char* name, int64_t dflt) {
  std::string v = envg(name, -1);
  return v.empty() ? dflt : strtoll(v.c_str(), nullptr, 10);
}

void setup() {
  if (S.ready) return;
  S.origin = env_i64("ORIGIN_NS", 0);
  S.cadence = env_i64("CADENCE_NS", S.cadence);
  S.ts_offset = env_i64("TS_OFFSET_NS", S.ts_offset);
  S.base = uint64_t(env_i64("ACC_BASE", int64_t(S.base)));
  std::string mode = envg("TS_MODE", -1);
  S.ts_mode = mode == "zero" ? 1 : mode == "ticks10" ? 2 : 0;
  int e = 0;
  double m = std::frexp(double(S.res), &e);  // res = m * 2^e, 0.5 <= m < 1, 24 significant bits
  S.res_m = int64_t(std::ldexp(m, 24));
  S.res_s = 24 - e;
  std::string blk = envg("BLOCK", -1);
  if (!blk.empty()) {
    char where[16] = "after";
    long long t = 0, d = 0;
    if (sscanf(blk.c_str(), "%lld:%lld:%15s", &t, &d, where) >= 2) {
      S.block_t = t;
      S.block_dur = d;
      S.block_after = strcmp(where, "before") != 0;
    }
  }
  int n = int(env_i64("NGPU", 1));
  S.gpus.resize(size_t(n));
  for (int g = 0; g < n; ++g) {
    Gpu& G = S.gpus[size_t(g)];
    std::string p = envg("POWER", g);
    if (p.empty()) p = "300";
    size_t pos = 0;
    bool first = true;
    while (pos <= p.size()) {
      size_t c = p.find(',', pos);
      std::string tok = p.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
      if (first) {
        G.sched.push_back({0, strtoll(tok.c_str(), nullptr, 10)});
        first = false;
      } else {
        long long t = 0, w = 0;
        if (sscanf(tok.c_str(), "%lld:%lld", &t, &w) == 2) G.sched.push_back({t, w});
      }
      if (c == std::string::npos) break;
      pos = c + 1;
    }
    std::string f = envg("FAIL", g);
    if (f == "always") {
      G.fail_always = true;
    } else if (!f.empty()) {
      long long a = 0, b = 0;
      if (sscanf(f.c_str(), "%lld:%lld", &a, &b) == 2) G.fail_a = a, G.fail_b = b;
    }
    std::string bk = envg("BACK", g);
    if (!bk.empty()) {
      long long t = 0, k = 0;
      if (sscanf(bk.c_str(), "%lld:%lld", &t, &k) == 2) G.back_t = t, G.back_counts = k;
    }
    std::string cp = envg("CURPOWER", g);
    G.have_cur = !cp.empty();
    if (G.have_cur) G.cur_power = uint32_t(strtoull(cp.c_str(), nullptr, 10));
    std::string sp = envg("SOCKPOWER", g);
    G.sock_power = sp.empty() ? 77 : strtoull(sp.c_str(), nullptr, 10);
    std::string gf = envg("GFX", g), um = envg("UMC", g), vr = envg("VRAM", g);
    G.gfx = gf.empty() ? 50 : uint32_t(strtoull(gf.c_str(), nullptr, 10));
    G.umc = um.empty() ? 25 : uint32_t(strtoull(um.c_str(), nullptr, 10));
    unsigned long long used = 1000, total = 4000;
    if (!vr.empty()) sscanf(vr.c_str(), "%llu:%llu", &used, &total);
    G.vram_used = uint32_t(used);
    G.vram_total = uint32_t(total);
    S.procs.push_back({AMDSMI_PROCESSOR_TYPE_AMD_GPU, g});
    if (g == 0 && env_i64("CPU_BETWEEN", 0)) S.procs.push_back({AMDSMI_PROCESSOR_TYPE_AMD_CPU, -1});
  }
  S.ready = true;
}

// nanojoules of GPU g from the origin to relative time r
int64_t energy_nj(const Gpu& G, int64_t r) {
  int64_t e = 0;
  for (size_t i = 0; i < G.sched.size() && G.sched[i].first < r; ++i) {
    int64_t end = i + 1 < G.sched.size() && G.sched[i + 1].first < r ? G.sched[i + 1].first : r;
    e += G.sched[i].second * (end - G.sched[i].first);
  }
  return e;
}

int64_t watts_at(const Gpu& G, int64_t r) {
  int64_t w = G.sched.front().second;
  for (const auto& s : G.sched)
    if (s.first <= r) w = s.second;
  return w;
}

Gpu* gpu_of(amdsmi_processor_handle h) {
  auto* p = static_cast<Proc*>(h);
  if (!S.ready || !p || p->type != AMDSMI_PROCESSOR_TYPE_AMD_GPU) return nullptr;
  return &S.gpus[size_t(p->gpu)];
}

void sleep_ns(int64_t d) {
  timespec req{time_t(d / 1000000000ll), long(d % 1000000000ll)};
  while (nanosleep(&req, &req) != 0) {
  }
}

}  // namespace

extern "C" {

amdsmi_status_t amdsmi_init(uint64_t) {
  setup();
  return S.origin > 0 ? AMDSMI_STATUS_SUCCESS : AMDSMI_STATUS_INVAL;
}

amdsmi_status_t amdsmi_shut_down() { return AMDSMI_STATUS_SUCCESS; }

amdsmi_status_t amdsmi_get_socket_handles(uint32_t* count, amdsmi_socket_handle* handles) {
  if (!S.ready || !count) return AMDSMI_STATUS_INVAL;
  if (handles && *count >= 1) handles[0] = &S;
  *count = 1;
  return AMDSMI_STATUS_SUCCESS;
}

amdsmi_status_t amdsmi_get_processor_handles(amdsmi_socket_handle sock, uint32_t* count,
                                             amdsmi_processor_handle* handles) {
  if (!S.ready || sock != &S || !count) return AMDSMI_STATUS_INVAL;
  if (handles)
    for (uint32_t i = 0; i < *count && i < S.procs.size(); ++i) handles[i] = &S.procs[i];
  *count = uint32_t(S.procs.size());
  return AMDSMI_STATUS_SUCCESS;
}

amdsmi_status_t amdsmi_get_processor_type(amdsmi_processor_handle h, processor_type_t* t) {
  if (!S.ready || !h || !t) return AMDSMI_STATUS_INVAL;
  *t = static_cast<Proc*>(h)->type;
  return AMDSMI_STATUS_SUCCESS;
}

amdsmi_status_t amdsmi_get_energy_count(amdsmi_processor_handle h, uint64_t* acc, float* res, uint64_t* ts) {
  Gpu* G = gpu_of(h);
  if (!G || !acc || !res || !ts) return AMDSMI_STATUS_INVAL;
  int64_t r = now_ns() - S.origin;
  const bool block = r >= S.block_t && !S.blocked.exchange(true);
  if (block && !S.block_after) {
    sleep_ns(S.block_dur);
    r = now_ns() - S.origin;
  }
  if (G->fail_always || (r >= G->fail_a && r < G->fail_b)) return AMDSMI_STATUS_NOT_SUPPORTED;
  if (r < 0) r = 0;
  const int64_t rq = r / S.cadence * S.cadence;
  const unsigned __int128 num = (unsigned __int128)(uint64_t(energy_nj(*G, rq))) << S.res_s;
  const unsigned __int128 den = (unsigned __int128)(1000) * uint64_t(S.res_m);  // nJ per count, scaled alike
  *acc = S.base + uint64_t(num / den) - (rq >= G->back_t ? uint64_t(G->back_counts) : 0);
  *res = S.res;
  const int64_t dev = S.origin + rq - S.ts_offset;
  *ts = S.ts_mode == 1 ? 0 : S.ts_mode == 2 ? uint64_t(dev / 10) : uint64_t(dev);
  if (block && S.block_after) sleep_ns(S.block_dur);
  return AMDSMI_STATUS_SUCCESS;
}

amdsmi_status_t amdsmi_get_power_info(amdsmi_processor_handle h, amdsmi_power_info_t* p) {
  Gpu* G = gpu_of(h);
  if (!G || !p) return AMDSMI_STATUS_INVAL;
  memset(p, 0, sizeof(*p));
  p->socket_power = G->sock_power;
  p->current_socket_power = G->have_cur ? G->cur_power : uint32_t(watts_at(*G, now_ns() - S.origin));
  p->average_socket_power = UINT32_MAX;
  return AMDSMI_STATUS_SUCCESS;
}

amdsmi_status_t amdsmi_get_gpu_activity(amdsmi_processor_handle h, amdsmi_engine_usage_t* a) {
  Gpu* G = gpu_of(h);
  if (!G || !a) return AMDSMI_STATUS_INVAL;
  memset(a, 0, sizeof(*a));
  a->gfx_activity = G->gfx;
  a->umc_activity = G->umc;
  a->mm_activity = UINT32_MAX;
  return AMDSMI_STATUS_SUCCESS;
}

amdsmi_status_t amdsmi_get_gpu_vram_usage(amdsmi_processor_handle h, amdsmi_vram_usage_t* v) {
  Gpu* G = gpu_of(h);
  if (!G || !v) return AMDSMI_STATUS_INVAL;
  memset(v, 0, sizeof(*v));
  v->vram_used = G->vram_used;
  v->vram_total = G->vram_total;
  return AMDSMI_STATUS_SUCCESS;
}

amdsmi_status_t amdsmi_get_gpu_device_bdf(amdsmi_processor_handle h, amdsmi_bdf_t* b) {
  auto* p = static_cast<Proc*>(h);
  if (!gpu_of(h) || !b) return AMDSMI_STATUS_INVAL;
  b->as_uint = 0;
  b->bus_number = uint64_t(0x10 + p->gpu);
  return AMDSMI_STATUS_SUCCESS;
}

}  // extern "C"
