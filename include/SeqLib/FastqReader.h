// FastqReader.h -- SeqLib::FastqReader for the MI355X drop-in: FASTA / FASTQ (plain or gzip) -> UnalignedSequence,
// the producer in front of BWAAligner::alignSequences (first "next" row).
// Same interface and return conventions as /root/reference/SeqLib/FastqReader.h:26-74 and
// /root/reference/src/FastqReader.cpp:8-59.  The reference delegates the parsing to bwa's kseq.h (un-vendored
// submodule); the record grammar is restated here as one small pull parser over a zlib stream:
//   * anything before the first '>' or '@' is skipped;
//   * the name runs to the first whitespace byte, the comment (if the name did not end the line) to the end of line;
//   * sequence lines are concatenated until a line STARTS with '>', '@' or '+'; empty lines are skipped;
//   * after '+', quality lines are concatenated until they are at least as long as the sequence; a length mismatch or
//     a missing quality block is an error and ends the stream (kseq_read() < 0  =>  GetNextSequence() == false);
//   * a '\r' before the line feed is dropped from comment/sequence/quality lines longer than one byte.
// Like the reference, a field of `s` is only assigned once the parser has a buffer for it: Com stays untouched until
// the first record with a comment line has been seen, Qual until the first '+' block (kseq's lazily allocated kstring).
//
// NextBatch (new) is the batch form of the same grammar: the file given to Open goes through the GPU parser of libseqlib_amd.so (seqlib_amd_fastq.h) and a
// batch comes out in HBM, laid out as BWAAligner::alignToBam(FastqReader&) hands it on, or copied down into an UnalignedSequenceVector.  One pass over a file
// is either per read or per batch: the first NextBatch after a GetNextSequence of the same pass, and a GetNextSequence after a NextBatch, throw
// std::logic_error; Open starts a new pass.  The batch handle is opened lazily, so a program that calls only Open and GetNextSequence needs no library.
#pragma once
#include <cctype>
#include <cstdint>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include "SeqLib/UnalignedSequence.h"
#include "seqlib_amd_fastq.h"

namespace SeqLib {

// one batch of NextBatch: slx_fastq_batch's arrays in HBM, valid until the reader's next call
struct FastqBatch {
    slx_fastq_batch dev = {};
    size_t size() const { return (size_t)dev.n_reads; }
    bool empty() const { return dev.n_reads == 0; }
};

class FastqReader {
public:
    FastqReader() = default;
    explicit FastqReader(const std::string &file) : m_file(file) { Open(m_file); }
    FastqReader(const FastqReader &) = delete;
    FastqReader &operator=(const FastqReader &) = delete;
    ~FastqReader() { if (fp_) gzclose(fp_); if (fq_) fq_close_(fq_); }

    // src/FastqReader.cpp:8-31: false (with a message on stderr) when the path does not stat or zlib cannot open it
    bool Open(const std::string &f)
    {
        m_file = f;
        struct stat st;
        if (stat(m_file.c_str(), &st) != 0) {
            std::cerr << "FastqReader: Failed to read non-existant file " << m_file << std::endl;
            return false;
        }
        if (fp_) { gzclose(fp_); fp_ = nullptr; }
        fp_ = (m_file != "-") ? gzopen(m_file.c_str(), "r") : gzdopen(fileno(stdin), "r");
        if (!fp_) {
            std::cerr << "FastqReader: Failed to read " << m_file << std::endl;
            return false;
        }
        gzbuffer(fp_, 1u << 18);
        begin_ = end_ = 0; eof_ = false; pending_ = 0;
        have_com_ = have_qual_ = false;
        return true;
    }

    // src/FastqReader.cpp:37-57
    bool GetNextSequence(UnalignedSequence &s)
    {
        if (!fp_) return false;
        if (parse_record() < 0) return false;
        s.Name = name_;
        if (have_com_) s.Com = com_;
        s.Seq = seq_;
        if (have_qual_) s.Qual = qual_;
        return true;
    }

    // ---- batches (new).  max_bytes: about that much text per batch (seqlib_amd_fastq.h).  False at the end of the input (and after a damaged tail, as
    // GetNextSequence); std::runtime_error when the library refuses (no GPU, a file it cannot read): there is no CPU fallback for batches.
    bool NextBatch(FastqBatch &out, size_t max_bytes = 64 << 20)
    {
        out = FastqBatch();
        if (!fp_) return false;
        if (begin_ != IN_BATCHES) {                         // the first batch since Open
            if (begin_ || end_ || eof_ || pending_) throw std::logic_error("FastqReader::NextBatch: GetNextSequence has begun this pass over the file; Open() starts a new one");
            if (fq_ && fq_file_ == m_file) { if (slx_fastq_rewind(fq_) != 0) throw std::runtime_error(std::string("FastqReader::NextBatch: ") + slx_last_error()); }
            else {
                if (fq_) { fq_close_(fq_); fq_ = nullptr; }
                if (slx_fastq_open(m_file.c_str(), -1, &fq_) != 0) { fq_ = nullptr; throw std::runtime_error(std::string("FastqReader::NextBatch: ") + slx_last_error()); }
                fq_close_ = &slx_fastq_close;
                fq_file_ = m_file;
            }
            begin_ = end_ = IN_BATCHES; eof_ = true;        // (Open resets the three)
        }
        if (slx_fastq_next(fq_, (int64_t)max_bytes, &out.dev) != 0) throw std::runtime_error(std::string("FastqReader::NextBatch: ") + slx_last_error());
        return out.dev.n_reads > 0;
    }
    // the same copied down: the reads a GetNextSequence loop over the batch's text pushes back, field by field
    bool NextBatch(UnalignedSequenceVector &out, size_t max_bytes = 64 << 20)
    {
        out.clear();
        FastqBatch b;
        if (!NextBatch(b, max_bytes)) return false;
        const size_t n = b.size();
        std::vector<uint64_t> ob(n + 1), on(n + 1), oc(n + 1);
        std::vector<uint8_t> fl(n);
        if (slx_fastq_to_host(fq_, &b.dev, nullptr, ob.data(), nullptr, nullptr, on.data(), nullptr, oc.data(), fl.data()) != 0) throw std::runtime_error(std::string("FastqReader::NextBatch: ") + slx_last_error());
        std::string bs(ob[n], '\0'), qs(ob[n], '\0'), ns(on[n], '\0'), cs(oc[n], '\0');
        if (slx_fastq_to_host(fq_, &b.dev, &bs[0], nullptr, &qs[0], &ns[0], nullptr, &cs[0], nullptr, nullptr) != 0) throw std::runtime_error(std::string("FastqReader::NextBatch: ") + slx_last_error());
        out.resize(n);
        for (size_t i = 0; i < n; ++i) {
            UnalignedSequence &u = out[i];
            u.Name.assign(ns, on[i], on[i + 1] - on[i]);
            u.Com.assign(cs, oc[i], oc[i + 1] - oc[i]);
            u.Seq.assign(bs, ob[i], ob[i + 1] - ob[i]);
            if (fl[i] & 2) u.Qual.assign(qs, ob[i], ob[i + 1] - ob[i]);
        }
        return true;
    }
    // slx_fastq_counter of the batch handle ("reads", "fast_reads", "slow_reads", "bad_tail", "source", "us_lines", ...); -1 before the first NextBatch
    int64_t BatchCounter(const char *name) const { return fq_ ? slx_fastq_counter(fq_, name) : -1; }

private:
    static constexpr int BUF = 1 << 16;
    static constexpr int IN_BATCHES = -1;                   // begin_ / end_ of a pass that NextBatch serves

    int getc_()
    {
        if (begin_ >= end_) {
            if (eof_) return -1;
            begin_ = 0;
            end_ = gzread(fp_, buf_, BUF);
            if (end_ < BUF) eof_ = true;
            if (end_ <= 0) { end_ = 0; return -1; }
        }
        return (unsigned char)buf_[begin_++];
    }
    // appends bytes up to (not including) the next delimiter; line mode stops at '\n', otherwise at any whitespace.
    // Returns the delimiter, or -1 when the input ended before any byte was seen.
    int until_(bool line, std::string &dst)
    {
        bool any = false;
        int c;
        while ((c = getc_()) != -1) {
            any = true;
            if (line ? c == '\n' : std::isspace(c) != 0) break;
            dst.push_back((char)c);
        }
        if (!any) return -1;
        if (line && dst.size() > 1 && dst.back() == '\r') dst.pop_back();
        return c == -1 ? 0 : c;
    }
    // >=0 sequence length; -1 end of input; -2 truncated / inconsistent quality
    int parse_record()
    {
        if (begin_ == IN_BATCHES) throw std::logic_error("FastqReader::GetNextSequence: NextBatch has begun this pass over the file; Open() starts a new one");
        int c;
        if (pending_ == 0) {
            while ((c = getc_()) != -1 && c != '>' && c != '@') {}
            if (c == -1) return -1;
            pending_ = c;
        }
        name_.clear(); com_.clear(); seq_.clear(); qual_.clear();
        const int d = until_(false, name_);
        if (d == -1) return -1;
        if (d != '\n' && until_(true, com_) != -1) have_com_ = true;
        while ((c = getc_()) != -1 && c != '>' && c != '+' && c != '@') {
            if (c == '\n') continue;
            seq_.push_back((char)c);
            until_(true, seq_);
        }
        if (c == '>' || c == '@') pending_ = c;
        if (c != '+') return (int)seq_.size();
        have_qual_ = true;
        while ((c = getc_()) != -1 && c != '\n') {}
        if (c == -1) return -2;
        while (until_(true, qual_) >= 0 && qual_.size() < seq_.size()) {}
        pending_ = 0;
        if (qual_.size() != seq_.size()) return -2;
        return (int)seq_.size();
    }

    std::string m_file;
    gzFile fp_ = nullptr;
    char buf_[BUF];
    int begin_ = 0, end_ = 0;
    bool eof_ = false;
    int pending_ = 0;           // header byte of the next record already consumed ('>' or '@'), 0 if none
    bool have_com_ = false, have_qual_ = false;
    std::string name_, com_, seq_, qual_;
    slx_fastq *fq_ = nullptr;                    // the batch handle, opened by the first NextBatch on fq_file_
    void (*fq_close_)(slx_fastq *) = nullptr;    // slx_fastq_close, taken when the handle is opened: the destructor names no library symbol
    std::string fq_file_;
};

}  // namespace SeqLib
