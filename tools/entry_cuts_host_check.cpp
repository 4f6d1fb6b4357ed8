// Stand-alone host check of the entry cuts, for sanitizer runs:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -pthread \
//       tools/entry_cuts_host_check.cpp \
//       ceng795_amd/csrc/{entry_cuts,scene_build,accel_build,scene_xml,xml_dom}.cpp \
//       -o entry_cuts_host_check && ./entry_cuts_host_check scene.xml [scene.xml ...]
// Every scene file named is loaded and built with its culling tree; every camera's table is built
// (build_entry_cuts, timed) and every pixel ray checked against it (check_entry_cuts).  With
// --no-check as the first argument only the build runs (its time on a large scene).
#include <chrono>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "../ceng795_amd/csrc/host_scene.h"

using namespace rt;

static double now_ms() {
  return std::chrono::duration<double, std::milli>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv) {
  int failures = 0, first = 1;
  bool check = true;
  if (argc > 1 && !std::strcmp(argv[1], "--no-check")) check = false, first = 2;
  if (first >= argc) {
    std::printf("usage: %s [--no-check] scene.xml ...\n", argv[0]);
    return 2;
  }
  for (int i = first; i < argc; i++) {
    try {
      XmlSceneStorage st;
      rt_scene_desc d;
      const double t0 = now_ms();
      load_scene_xml(argv[i], st, d);
      HostScene h;
      build_host_scene(d, h);
      const double t1 = now_ms();
      build_accel(h, kDefaultTreeletLeaves);
      const double t2 = now_ms();
      std::printf("%s: load + reference tree %.1f ms, culling tree %.1f ms\n", argv[i], t1 - t0,
                  t2 - t1);
      if (!entry_cuts_apply(h, kLaneStack - 2)) {
        std::printf("  no entry cuts for this scene\n");
        continue;
      }
      for (size_t cam = 0; cam < h.cameras.size(); cam++) {
        long long stats[kEntryCutStats];
        const double t3 = now_ms();
        const std::vector<int> table = build_entry_cuts(h, h.cameras[cam], stats);
        const double t4 = now_ms();
        std::printf("  camera %zu: %lld tiles, table %.1f ms; by size", cam, stats[kEcTiles], t4 - t3);
        for (int n = 1; n <= kEntryCut; n++) std::printf(" %lld", stats[kEcBySize + n]);
        std::printf("; by depth");
        for (int k = 0; k < kEntryCutDepths; k++) std::printf(" %lld", stats[kEcByDepth + k]);
        std::printf("; to root %lld; visits above %lld, slots above %lld\n", stats[kEcToRoot],
                    stats[kEcSavedVisits], stats[kEcSavedSlots]);
        if (!check) continue;
        long long where[4] = {0, 0, 0, 0};
        const long long bad = check_entry_cuts(h, h.cameras[cam], table, where);
        if (bad != 0) {
          std::printf("FAILED %s camera %zu: %lld violations, first at pixel %lld %lld node %lld slot %lld\n",
                      argv[i], cam, bad, where[0], where[1], where[2], where[3]);
          failures++;
        }
      }
    } catch (const std::exception& e) {
      std::printf("FAILED %s: %s\n", argv[i], e.what());
      failures++;
    }
  }
  std::printf(failures ? "%d FAILED\n" : "all passed\n", failures);
  return failures ? 1 : 0;
}
