// gm_property_of_collection.h -- a node property whose values are collections (`N_P<Node_Set>`), as it appears in an
// emitted signature (gm_cpp_gen.cc:1001: `gm_property_of_collection<T>&`) and in a driver
// (potential_friends_main.cc:7,17: `new gm_property_of_collection_impl<gm_node_set, false>(G.num_nodes())`; the reference's
// class: apps/output_cpp/gm_graph/inc/gm_property_of_collection.h:17-71).  size collections, each constructed with `size` as
// its maximum; lazy = true constructs a collection on its first use.
#ifndef GM_PROPERTY_OF_COLLECTION_H_
#define GM_PROPERTY_OF_COLLECTION_H_
#include <stddef.h>
#include <vector>

class gm_complex_data_type
{
  public:
    virtual ~gm_complex_data_type() {}
};

template <class T>
class gm_property_of_collection : public gm_complex_data_type
{
  public:
    virtual T& operator[](int index) = 0;
    virtual ~gm_property_of_collection() {}
};

template <class T, bool lazy>
class gm_property_of_collection_impl : public gm_property_of_collection<T>
{
  public:
    explicit gm_property_of_collection_impl(int size) : size_(size), data_((size_t) (size > 0 ? size : 0), (T*) NULL) {
        if (!lazy)
            for (size_t i = 0; i < data_.size(); i++) data_[i] = new T((size_t) size_);
    }
    ~gm_property_of_collection_impl() {
        for (size_t i = 0; i < data_.size(); i++) delete data_[i];
    }
    T& operator[](int index) {
        if (lazy && data_[(size_t) index] == NULL) {
#pragma omp critical(gm_property_of_collection_lazy)
            if (data_[(size_t) index] == NULL) data_[(size_t) index] = new T((size_t) size_);
        }
        return *data_[(size_t) index];
    }

  private:
    gm_property_of_collection_impl(const gm_property_of_collection_impl&);
    gm_property_of_collection_impl& operator=(const gm_property_of_collection_impl&);
    int size_;
    std::vector<T*> data_;
};
#endif
