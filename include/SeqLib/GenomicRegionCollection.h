// GenomicRegionCollection.h -- SeqLib::GenomicRegionCollection<T> and GRC for the MI355X drop-in: the container side of
// /root/reference/SeqLib/GenomicRegionCollection.h that BamReader::SetRegions needs -- add, size, operator[] / at, begin / end, clear, IsEmpty.
// The interval-tree side of the reference class (CreateTreeMap, FindOverlaps, FindOverlapWidth, CountOverlaps, CountContained, FindOverlappedIntervals,
// MergeOverlappingIntervals, Intersection, Concat, CoordinateSort, SortAndStretch*, Shuffle, Pad, ReadBED / ReadVCF, Total/Width sums) is not carried
// and is not declared: code that uses it fails to compile rather than getting an empty answer.
#pragma once
#include <cstddef>
#include <stdexcept>
#include <vector>
#include "SeqLib/GenomicRegion.h"

namespace SeqLib {

template <typename T = GenomicRegion> class GenomicRegionCollection {
public:
    typedef typename std::vector<T>::iterator iterator;
    typedef typename std::vector<T>::const_iterator const_iterator;

    GenomicRegionCollection() = default;
    explicit GenomicRegionCollection(const std::vector<T> &vec) : v_(vec) {}
    explicit GenomicRegionCollection(const T &gr) : v_(1, gr) {}

    void add(const T &g) { v_.push_back(g); }
    size_t size() const { return v_.size(); }
    bool IsEmpty() const { return v_.empty(); }
    void clear() { v_.clear(); }
    // unchecked, as a vector's; at() throws out_of_range
    const T &operator[](size_t i) const { return v_[i]; }
    T &operator[](size_t i) { return v_[i]; }
    const T &at(size_t i) const
    {
        if (i >= v_.size()) throw std::out_of_range("GenomicRegionCollection::at - index out of range");
        return v_[i];
    }
    iterator begin() { return v_.begin(); }
    iterator end() { return v_.end(); }
    const_iterator begin() const { return v_.begin(); }
    const_iterator end() const { return v_.end(); }
    const std::vector<T> &AsGenomicRegionVector() const { return v_; }

private:
    std::vector<T> v_;
};

typedef GenomicRegionCollection<GenomicRegion> GRC;

}  // namespace SeqLib
