// viekf_host.hpp -- host-side declarations shared by the C-ABI implementation files.
#pragma once
#include <map>
#include <string>
#include <vector>

namespace viekf {

typedef std::map<std::string, std::string> YamlMap;
bool yaml_parse_file(const std::string& path, YamlMap& out, std::string& err);
bool yaml_get_doubles(const YamlMap& m, const std::string& key, double* out, int count, std::string& err);
bool yaml_get_string(const YamlMap& m, const std::string& key, std::string& out, std::string& err);
// records `msg` as this thread's viekf_last_error() and returns `code` (defined in viekf_capi.hip, used by every C-ABI file)
int set_last_error(int code, const std::string& msg);
// block ownership map [RB][64 * NWV] of the fused-step kernel (viekf_resmap.cpp); false when the blocks do not fit
bool build_resmap(int N, int RB, int NWV, std::vector<int>& map, int* used_slots = nullptr);
// its last pass (lanes permuted inside the groups): the (thread, feature) repeats left on worker wave w, and the assignment solver
int resmap_wave_repeats(const std::vector<int>& map, int RB, int NWV, int w);
std::vector<int> resmap_assign(const std::vector<std::vector<long>>& cost);

// Column stride of P for num_features features (viekf_batch_create explains the choice)
inline int cov_ld(int num_features) {
  const int n = 16 + 3 * num_features;
#ifdef VIEKF_LD_PAD_ALL               // (diagnostic build, tools/build_variant.sh: A/B of the padded stride on the on-chip family)
  return (n + 15) & ~15;
#endif
  return num_features > 77 ? (n + 15) & ~15 : (n + 1) & ~1;
}

}  // namespace viekf
