// gm_set.h -- Node_Set / Edge_Set as they appear in an emitted signature (`N_P<Node_Set>` ->
// `gm_property_of_collection<gm_node_set>&`; the reference's container: apps/output_cpp/gm_graph/inc/gm_set.h:9-388).
// The part of its interface that a driver (potential_friends_main.cc:25-38: copy, prepare_seq_iteration, has_next /
// get_next) and an entry point touch.  The reference switches between a std::set and a byte map of max_sz entries; both
// iterate in ascending order.  Here a set is one sorted vector: it holds only its members, so a property of V sets costs
// what the results cost, not V bytes per vertex.
#ifndef GM_SET_H_
#define GM_SET_H_
#include <stddef.h>
#include <algorithm>
#include <vector>
#include "gm_graph_typedef.h"

template <typename T>
class gm_sized_set
{
  public:
    explicit gm_sized_set(size_t max_sz = 0) : max_sz_(max_sz) {}

    bool is_in(T e) const { return std::binary_search(items_.begin(), items_.end(), e); }
    void add(T e) {
        typename std::vector<T>::iterator at = std::lower_bound(items_.begin(), items_.end(), e);
        if (at == items_.end() || *at != e) items_.insert(at, e);
    }
    void remove(T e) {
        typename std::vector<T>::iterator at = std::lower_bound(items_.begin(), items_.end(), e);
        if (at != items_.end() && *at == e) items_.erase(at);
    }
    void clear() { items_.clear(); }
    size_t get_size() const { return items_.size(); }
    size_t get_max_size() const { return max_sz_; }
    // This project's extension: the whole set at once from n ascending, distinct values (what the device returns).
    void assign_sorted(const T* sorted, size_t n) { items_.assign(sorted, sorted + n); }

    class seq_iter
    {
      public:
        seq_iter() : cur_(NULL), end_(NULL) {}
        seq_iter(const T* b, const T* e) : cur_(b), end_(e) {}
        bool has_next() const { return cur_ != end_; }
        T get_next() { return *cur_++; }
      private:
        const T *cur_, *end_;
    };
    typedef seq_iter par_iter;
    // ascending; valid until the set changes
    seq_iter prepare_seq_iteration() const { return seq_iter(items_.data(), items_.data() + items_.size()); }
    par_iter prepare_par_iteration(int thread_id, int /*max_threads*/) const {
        return thread_id == 0 ? prepare_seq_iteration() : seq_iter(items_.data() + items_.size(), items_.data() + items_.size());
    }

  private:
    size_t max_sz_;
    std::vector<T> items_;
};

typedef gm_sized_set<node_t> gm_node_set;
typedef gm_sized_set<edge_t> gm_edge_set;
#endif
