// recsort_host.h -- the one copy of the header rule of a coordinate sort (slx_sort_header, include/seqlib_amd_sort.h): host only.
//   an @HD line with an SO: field   its value becomes "coordinate"; every other field, and the field order, is kept
//   an @HD line without SO:         "\tSO:coordinate" is appended
//   a text without @HD              "@HD\tVN:1.6\tSO:coordinate\n" goes in front
// @HD is only looked for as the first line, where SAMv1 1.3 places it.
#pragma once
#include <algorithm>
#include <string>

static inline std::string recsort_header_so(const std::string &text)
{
    if (text.compare(0, 3, "@HD") != 0 || (text.size() > 3 && text[3] != '\t' && text[3] != '\n')) return "@HD\tVN:1.6\tSO:coordinate\n" + text;
    size_t eol = text.find('\n');
    if (eol == std::string::npos) eol = text.size();
    for (size_t p = 3; p < eol; ) {          // p: at a tab
        const size_t q = std::min(text.find('\t', p + 1), eol);
        if (text.compare(p + 1, 3, "SO:") == 0) return text.substr(0, p + 4) + "coordinate" + text.substr(q);
        p = q;
    }
    return text.substr(0, eol) + "\tSO:coordinate" + text.substr(eol);
}
