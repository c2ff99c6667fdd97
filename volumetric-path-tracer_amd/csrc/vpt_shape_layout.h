// vpt_shape_layout.h — the integer half of vpt_scene_update_shapes (include/vpt.h): the new shape list, the renumbering
// and the offsets of every shape in a pool.  Plain C++ over no HIP header, so that it can be checked on a machine without a device.
#pragma once
#include <cstddef>
#include <vector>

// one entry of the new shape list: the old id of a survivor (-1: an added shape) and the entry of the edit's payload - the `set`
// entries, then the added ones - that holds its mesh (-1: an untouched survivor, which keeps its part of every pool)
struct shape_slot { int old_id = -1, payload = -1; };

// The old list with the `set` entries marked, the removed ones erased and `num_add` entries appended: survivors keep their order and
// the ids close up.  new_of_old[i] = the new id of old shape i, -1: removed.  The ids are the caller's checked ones (in range, no
// repeats, none both set and removed).
void shape_list_of_edit(int num_old, const int* remove_ids, int num_remove, const int* set_ids, int num_set, int num_add, std::vector<shape_slot>& list,
    std::vector<int>& new_of_old);

// where every shape starts in a pool that is contiguous in shape order: the exclusive prefix sums of `lengths`, and the total as the
// last of n + 1 entries
std::vector<long long> pool_offsets(const std::vector<long long>& lengths);

// maximal runs of untouched survivors that are adjacent in the old list and in the new one: `count` shapes from first_old on become
// the shapes from first_new on, so their part of a pool moves in one copy
struct shape_run { int first_new, first_old, count; };
std::vector<shape_run> survivor_runs(const std::vector<shape_slot>& list);
