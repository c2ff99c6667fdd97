// vpt_shape_layout.cpp — the new shape list, the renumbering and the pool offsets of vpt_scene_update_shapes (vpt_shape_layout.h)
#include "vpt_shape_layout.h"

void shape_list_of_edit(int num_old, const int* remove_ids, int num_remove, const int* set_ids, int num_set, int num_add, std::vector<shape_slot>& list,
    std::vector<int>& new_of_old) {
  std::vector<char> keep((size_t)num_old, 1);
  std::vector<int>  payload((size_t)num_old, -1);
  for (int i = 0; i < num_remove; i++) keep[(size_t)remove_ids[i]] = 0;
  for (int i = 0; i < num_set; i++) payload[(size_t)set_ids[i]] = i;
  list.clear(), new_of_old.assign((size_t)num_old, -1);
  for (int i = 0; i < num_old; i++) {
    if (!keep[(size_t)i]) continue;
    new_of_old[(size_t)i] = (int)list.size();
    list.push_back({i, payload[(size_t)i]});
  }
  for (int i = 0; i < num_add; i++) list.push_back({-1, num_set + i});
}

std::vector<long long> pool_offsets(const std::vector<long long>& lengths) {
  std::vector<long long> at(lengths.size() + 1, 0);
  for (size_t i = 0; i < lengths.size(); i++) at[i + 1] = at[i] + lengths[i];
  return at;
}

std::vector<shape_run> survivor_runs(const std::vector<shape_slot>& list) {
  std::vector<shape_run> runs;
  for (int j = 0; j < (int)list.size(); j++) {
    const shape_slot& s = list[(size_t)j];
    if (s.old_id < 0 || s.payload >= 0) continue;
    if (!runs.empty() && runs.back().first_new + runs.back().count == j && runs.back().first_old + runs.back().count == s.old_id) runs.back().count++;
    else runs.push_back({j, s.old_id, 1});
  }
  return runs;
}
