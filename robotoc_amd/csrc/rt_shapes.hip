// rt_shapes.hip -- the kernel sets of the runtime: the compiled-in table of robot shapes and the plugin loader.
#include <dlfcn.h>

#include <mutex>

#include "rt_context.hpp"

using namespace rtoc;

// ---- kernel table: one entry per compiled robot shape (shape_inst.hip; SHAPES in the Makefile) ------------
#define RTOC_SHAPE(nv, nu, ns, nw0, nw1) namespace rtoc { KernelSet rtoc_shape_##nv##_##nu##_##ns(); }
#include "shape_table.inc"
#undef RTOC_SHAPE
static const std::vector<KernelSet>& kernel_table() {
  static std::vector<KernelSet> t = {
#define RTOC_SHAPE(nv, nu, ns, nw0, nw1) rtoc::rtoc_shape_##nv##_##nu##_##ns(),
#include "shape_table.inc"
#undef RTOC_SHAPE
  };
  return t;
}

// Shapes beyond the compiled-in table: librtoc_shape_<nv>_<nu>_<ns>.so next to this library (or in $RTOC_SHAPE_DIR),
// built by `make -C robotoc_amd/csrc plugin SHAPE=nv:nu:ns:nw0:nw1`; with RTOC_SHAPE_JIT=1 rtoc_create builds it itself, next to
// this library wherever it lives now (hipcc + the source directory this library was built from must be present; ~1 min, once).

static std::vector<KernelSet>& plugin_table() {
  static std::vector<KernelSet> t;
  return t;
}
static std::string library_dir() {
  Dl_info info;
  if (dladdr((const void*)&library_dir, &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    const size_t k = p.find_last_of('/');
    return k == std::string::npos ? std::string(".") : p.substr(0, k);
  }
  return ".";
}
static const KernelSet* load_plugin(const rtoc_dims* d) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  for (const auto& k : plugin_table())
    if (k.nv == d->nv && k.nu == d->nu && k.ns == d->ns_max) return &k;
  char name[96];
  snprintf(name, sizeof name, "librtoc_shape_%d_%d_%d.so", d->nv, d->nu, d->ns_max);
  std::vector<std::string> dirs;
  if (const char* e = getenv("RTOC_SHAPE_DIR")) dirs.push_back(e);
  dirs.push_back(library_dir());
  void* h = nullptr;
  for (const auto& dir : dirs)
    if ((h = dlopen((dir + "/" + name).c_str(), RTLD_NOW | RTLD_LOCAL))) break;
#ifdef RTOC_CSRC_DIR
  const char* jit = getenv("RTOC_SHAPE_JIT");
  if (!h && jit && jit[0] == '1') {
    // tile-split wave counts by state dimension, like the compiled-in shapes: one / three waves up to 36, four beyond
    const int nx = 2 * d->nv, nw0 = nx <= 36 ? 1 : 4, nw1 = nx <= 36 ? 3 : (nx > 64 ? 5 : 4);
    char shape[96];
    snprintf(shape, sizeof shape, "SHAPE=%d:%d:%d:%d:%d", d->nv, d->nu, d->ns_max, nw0, nw1);
    const std::string cmd = std::string("make -s -C '") + RTOC_CSRC_DIR + "' plugin " + shape + " PLUGIN_DIR='" + library_dir() + "' >/dev/null 2>&1";
    if (system(cmd.c_str()) == 0) h = dlopen((library_dir() + "/" + name).c_str(), RTLD_NOW | RTLD_LOCAL);
  }
#endif
  if (!h) return nullptr;
  typedef int (*entry_t)(KernelSet*, size_t, size_t);
  entry_t entry = (entry_t)dlsym(h, "rtoc_shape_plugin");
  KernelSet k;
  if (!entry || entry(&k, sizeof(KernelSet), kernel_abi_stamp()) != 0 || k.nv != d->nv || k.nu != d->nu || k.ns != d->ns_max) {
    dlclose(h);
    return nullptr;
  }
  plugin_table().reserve(64);  // handed-out pointers stay valid
  if (plugin_table().size() >= 64) return nullptr;
  plugin_table().push_back(k);
  return &plugin_table().back();
}

const KernelSet* rtoc::find_set(const rtoc_dims* d) {
  if (d->nf_max != d->ns_max || d->np != d->nv - d->nu) return nullptr;
  for (const auto& k : kernel_table())
    if (k.nv == d->nv && k.nu == d->nu && k.ns == d->ns_max) return &k;
  return load_plugin(d);
}
