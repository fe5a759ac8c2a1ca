// The order rules of a series run's rank-0 sink, where the multi-frame engine delivers columns out of order: InOrder
// hands items out in frame order (/solution is written in time order), ColumnCount tells when the last column of a
// composite frame has come (--beta_scan, --replicas: virtual frame j = k nc + column). Host code only.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace sart {

template <class Item>
class InOrder {
   public:
    explicit InOrder(int64_t first = 0) : next_(first) {}  // first: the first index handed out (below it: never)
    void put(int64_t k, Item item) { held_.emplace(k, std::move(item)); }
    // emit(k, Item&&) for every held item whose index is the next one, in order
    template <class Emit>
    void drain(Emit&& emit) {
        for (auto it = held_.find(next_); it != held_.end(); it = held_.find(next_)) {
            Item item = std::move(it->second);
            held_.erase(it);
            emit(next_++, std::move(item));
        }
    }
    bool empty() const { return held_.empty(); }

   private:
    std::map<int64_t, Item> held_;
    int64_t next_;
};

class ColumnCount {
   public:
    ColumnCount(int64_t frames, int64_t nc) : nc_(nc), left_((size_t)frames, nc) {}
    int64_t frame(int64_t j) const { return j / nc_; }
    int64_t column(int64_t j) const { return j % nc_; }
    bool arrived(int64_t j) { return --left_[(size_t)frame(j)] == 0; }  // true: frame(j)'s last column (any order)

   private:
    const int64_t nc_;
    std::vector<int64_t> left_;  // columns of each composite frame still to come
};

}  // namespace sart
