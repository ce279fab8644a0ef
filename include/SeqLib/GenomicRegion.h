// GenomicRegion.h -- SeqLib::GenomicRegion for the MI355X drop-in: an interval on a reference (chr id, pos1, pos2, strand), the argument of
// BamReader::SetRegion / SetRegions.  Same members, signatures and exceptions as /root/reference/SeqLib/GenomicRegion.h:19-172 with
// /root/reference/src/GenomicRegion.cpp; header-only here.  The samtools-style string constructor restates htslib's hts_parse_reg (htslib is not part
// of this image): "name", "name:beg", "name:beg-end" with commas allowed in the numbers, the last ':' dividing name and range, and a string whose
// tail is not a range taken as a name as it stands; pos1 = beg + 1 and pos2 = end as src/GenomicRegion.cpp:166-168, a bare name giving the whole contig
// (pos1 = 1, pos2 = its length).  One difference on purpose: "name:beg" runs to the contig's end, where the reference looks the whole string up as a
// name and ends with chr = -1.
#pragma once
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>
#include "SeqLib/BamHeader.h"

namespace SeqLib {

class GenomicRegion {
    template <typename T> friend class GenomicRegionCollection;
public:
    GenomicRegion() : chr(-1), pos1(0), pos2(0), strand('*') {}
    GenomicRegion(int32_t t_chr, int32_t t_pos1, int32_t t_pos2, char t_strand = '*') : chr(t_chr), pos1(t_pos1), pos2(t_pos2), strand(t_strand)
    {
        if (t_pos2 < t_pos1) throw std::invalid_argument("GenomicRegion constructor: end pos must be >= start pos");
        if (t_strand != '+' && t_strand != '-' && t_strand != '*') throw std::invalid_argument("GenomicRegion constructor: strand must be one of +, -, *");
    }
    // positions as strings (std::stoi: invalid_argument / out_of_range); without a header "1" -> 0, "chr2" -> 1, "X" -> 22, "Y" -> 23
    GenomicRegion(const std::string &tchr, const std::string &tpos1, const std::string &tpos2, const BamHeader &hdr) : strand('*')
    {
        pos1 = std::stoi(tpos1);
        pos2 = std::stoi(tpos2);
        const std::string bare = tchr.compare(0, 3, "chr") == 0 ? tchr.substr(3) : tchr;
        if (hdr.isEmpty()) {
            chr = bare == "X" ? 22 : bare == "Y" ? 23 : std::stoi(bare) - 1;
            return;
        }
        chr = hdr.Name2ID(tchr);
        if (chr == -1 && !tchr.empty() && tchr.find_first_not_of("0123456789XY") == std::string::npos) chr = hdr.Name2ID("chr" + tchr);          // b37 names against an hg dictionary
    }
    // samtools-style: "chr7:10,000-11,100", "chr7:10,000", "chr7"
    GenomicRegion(const std::string &reg, const BamHeader &hdr) : strand('*')
    {
        if (hdr.isEmpty()) throw std::invalid_argument("GenomicRegion constructor - supplied empty BamHeader");
        std::string name;
        int64_t beg = 0, end = INT_MAX;
        if (hdr.Name2ID(reg) >= 0) name = reg;          // a contig's name as it stands, colons and all
        else if (!parse_region(reg, name, beg, end) || hdr.Name2ID(name) < 0) throw std::invalid_argument("GenomicRegion constructor: Failed to set region for " + reg);
        chr = hdr.Name2ID(name);
        if (end == INT_MAX) end = hdr.GetSequenceLength(chr);
        pos1 = (int32_t)beg + 1;
        pos2 = (int32_t)end;
    }

    bool IsEmpty() const { return chr == -1 && pos1 == 0 && pos2 == 0; }
    int Width() const { return pos2 - pos1 + 1; }          // inclusive
    int32_t DistanceBetweenStarts(const GenomicRegion &gr) const { return gr.chr != chr ? -1 : std::abs(pos1 - gr.pos1); }
    int32_t DistanceBetweenEnds(const GenomicRegion &gr) const { return gr.chr != chr ? -1 : std::abs(pos2 - gr.pos2); }
    void Pad(int32_t pad)
    {
        if (-2 * (int64_t)pad > Width())
            throw std::out_of_range("GenomicRegion::pad - negative pad values can't obliterate GenomicRegion with val " + std::to_string(chr) + ":" + std::to_string(pos1) + "-" +
                                    std::to_string(pos2) + " and pad " + std::to_string(pad));
        pos1 -= pad;
        pos2 += pad;
    }
    // 3: the argument contains this; 2: this contains the argument; 1: they overlap in part; 0: not at all (ends inclusive)
    int GetOverlap(const GenomicRegion &gr) const
    {
        if (gr.chr != chr || gr.pos2 < pos1 || gr.pos1 > pos2) return 0;
        if (gr.pos1 <= pos1 && pos2 <= gr.pos2) return 3;
        if (pos1 <= gr.pos1 && gr.pos2 <= pos2) return 2;
        return 1;
    }
    // by chr, then pos1, then pos2; the strand takes no part
    bool operator<(const GenomicRegion &b) const { return chr != b.chr ? chr < b.chr : pos1 != b.pos1 ? pos1 < b.pos1 : pos2 < b.pos2; }
    bool operator==(const GenomicRegion &b) const { return chr == b.chr && pos1 == b.pos1 && pos2 == b.pos2; }
    bool operator!=(const GenomicRegion &b) const { return !(*this == b); }
    bool operator>(const GenomicRegion &b) const { return b < *this; }
    bool operator<=(const GenomicRegion &b) const { return !(b < *this); }
    bool operator>=(const GenomicRegion &b) const { return !(*this < b); }

    // the name from the header; without one the default naming (id 0 -> "1", 22 -> "X", 23 -> "Y", 24 -> "M")
    std::string ChrName(const BamHeader &h) const
    {
        if (h.isEmpty()) return chrToString(chr);
        if (chr >= h.NumSequences()) throw std::invalid_argument("GenomicRegion::ChrName - not enough targets in BamHeader to cover ref id");
        return h.IDtoName(chr);
    }
    std::string ToString(const BamHeader &h) const { return ChrName(h) + ":" + commas(pos1) + "-" + commas(pos2) + "(" + strand + ")"; }
    std::string PointString(const BamHeader &h) const { return ChrName(h) + ":" + commas(pos1) + "(" + strand + ")"; }
    friend std::ostream &operator<<(std::ostream &out, const GenomicRegion &gr)
    {
        return out << gr.chrToString(gr.chr) << ":" << commas(gr.pos1) << "-" << commas(gr.pos2) << "(" << gr.strand << ")";
    }

    int32_t chr;
    int32_t pos1;
    int32_t pos2;
    char strand;          // one of * - +

private:
    static std::string commas(int32_t v)
    {
        std::string s = std::to_string(v);
        for (int i = (int)s.size() - 3; i > (v < 0 ? 1 : 0); i -= 3) s.insert((size_t)i, ",");
        return s;
    }
    std::string chrToString(int32_t ref) const { return ref == 22 ? "X" : ref == 23 ? "Y" : ref == 24 ? "M" : ref < 0 ? std::to_string(ref) : std::to_string(ref + 1); }
    // "name[:beg[-end]]" -> name, 0-based beg, end (INT_MAX: none given); false for a range that does not parse as one or runs backwards
    static bool parse_region(const std::string &reg, std::string &name, int64_t &beg, int64_t &end)
    {
        name = reg; beg = 0; end = INT_MAX;
        const size_t colon = reg.rfind(':');
        if (reg.empty()) return false;
        if (colon == std::string::npos) return true;
        std::string num[2];
        int k = 0;
        for (size_t i = colon + 1; i < reg.size(); ++i) {
            const char c = reg[i];
            if (c == ',') continue;
            if (c == '-' && k == 0 && !num[0].empty()) { k = 1; continue; }
            if (c < '0' || c > '9' || num[k].size() > 10) return true;          // not a range: the colon is part of the name
            num[k] += c;
        }
        if (num[0].empty() || (k == 1 && num[1].empty())) return true;
        name = reg.substr(0, colon);
        beg = std::atoll(num[0].c_str()) - 1;
        if (beg < 0) beg = 0;
        if (k == 1) end = std::atoll(num[1].c_str());
        if (end > INT_MAX) end = INT_MAX;
        return beg < end;
    }
};

typedef std::vector<GenomicRegion> GenomicRegionVector;

}  // namespace SeqLib
