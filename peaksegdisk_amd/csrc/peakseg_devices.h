/* peakseg_devices.h -- which GPU a call uses, and the per-thread state of a call fanned out over
 * several (PEAKSEG_HIP_DEVICES; the fan-out itself is in peakseg_fanout.h). */
namespace {

/* A shard thread of a fanned-out call: the device it is pinned to (-1 elsewhere).  Its nested
 * file-level calls solve there and do not fan out again. */
thread_local int g_shard_device = -1;

/* PEAKSEG_HIP_DEVICES: the devices the batch entry points deal their programs to, "all" or a
 * comma-separated list of ids (an id may repeat: its sets then run one after the other).
 * Unset or empty: 0 and no devices.  A malformed list or an id that is not visible:
 * ERROR_NO_HIP_DEVICE, with the offending entry and the visible count in last_error. */
int env_devices(std::vector<int> &devices) {
  devices.clear();
  const char *e = getenv("PEAKSEG_HIP_DEVICES");
  if (!e || !*e) return 0;
  const int visible = peakseg_hip_device_count();
  if (strcmp(e, "all") == 0) {
    for (int d = 0; d < visible; d++) devices.push_back(d);
    if (devices.empty()) {
      set_error("PEAKSEG_HIP_DEVICES=all: no HIP device visible (this library has no CPU fallback)");
      return ERROR_NO_HIP_DEVICE;
    }
    return 0;
  }
  for (const char *p = e;; p++) {
    char *end = nullptr;
    errno = 0;
    const long d = isdigit((unsigned char)*p) ? strtol(p, &end, 10) : -1;
    if (d < 0 || d > INT_MAX || errno || (*end != ',' && *end != 0)) {
      devices.clear();
      set_error("PEAKSEG_HIP_DEVICES=%s is not \"all\" or a comma-separated list of device ids "
                "(%d HIP devices visible)", e, visible);
      return ERROR_NO_HIP_DEVICE;
    }
    devices.push_back((int)d);
    p = end;
    if (*p == 0) break;
  }
  for (int d : devices)
    if (d >= visible) {
      devices.clear();
      set_error("PEAKSEG_HIP_DEVICES=%s: no HIP device %d visible (%d HIP devices visible)", e, d,
                visible);
      return ERROR_NO_HIP_DEVICE;
    }
  return 0;
}

/* which GPU a single problem set of the file-level entry points uses: a shard thread's own
 * device; else the first of PEAKSEG_HIP_DEVICES; else PEAKSEG_HIP_DEVICE (one process per GPU
 * sets it from its rank), default 0.  ERROR_NO_HIP_DEVICE when PEAKSEG_HIP_DEVICES is bad. */
int env_device(int &device) {
  device = 0;
  if (g_shard_device >= 0) {
    device = g_shard_device;
    return 0;
  }
  std::vector<int> devices;
  const int st = env_devices(devices);
  if (st || !devices.empty()) {
    if (!st) device = devices[0];
    return st;
  }
  if (const char *e = getenv("PEAKSEG_HIP_DEVICE")) {
    int d = atoi(e);
    if (d >= 0) device = d;
  }
  return 0;
}

/* One process-wide mutex per device id: a shard holds its device's from the creation of its
 * problem set to its destruction, so that no two sets of this process run on one device at the
 * same time (a solve's hipFree and arena growth synchronise the device). */
std::mutex &device_mutex(int device) {
  static std::mutex guard;
  static std::map<int, std::unique_ptr<std::mutex>> locks;
  std::lock_guard<std::mutex> lk(guard);
  std::unique_ptr<std::mutex> &m = locks[device];
  if (!m) m.reset(new std::mutex);
  return *m;
}

/* What the calling thread's last file-level call did with PEAKSEG_HIP_DEVICES
 * (peakseg_hip_last_fanout): one row per shard, and the shard of each entry (-1: none). */
struct FanoutReport {
  std::vector<int> device, programs;
  std::vector<double> seconds;
  std::vector<int> entry_shard;

  void clear(int n_entries) {
    device.clear();
    programs.clear();
    seconds.clear();
    entry_shard.assign((size_t)(n_entries > 0 ? n_entries : 0), -1);
  }
};
thread_local FanoutReport g_fanout;

/* A shard's device time, accumulated by every problem set it creates */
struct ShardClock {
  int programs = 0;
  double create_s = 0.0, solve_s = 0.0, fetch_s = 0.0;
  double seconds() const { return create_s + solve_s + fetch_s; }
};
thread_local ShardClock *g_shard_clock = nullptr;

}  // namespace
