// BamWriter.h -- SeqLib::BamWriter for the MI355X drop-in: the consumer behind BWAAligner ("next" row):
// writes the records alignSequence(s) produced as SAM text or as BAM (BGZF-framed, zlib deflate).
// Same interface and return conventions as /root/reference/SeqLib/BamWriter.h:10-136 and
// /root/reference/src/BamWriter.cpp:10-113 (false instead of exceptions; messages on stderr; Open refuses to
// reopen; WriteHeader needs a non-empty header and an open file).  The reference hands the bytes to htslib
// (hts_open / sam_hdr_write / sam_write1), which is not part of this image; the two encodings are restated from the
// SAM/BAM specification (SAMv1 sections 1.4, 4.1, 4.2):
//   SAM  : QNAME FLAG RNAME POS+1 MAPQ CIGAR RNEXT PNEXT+1 TLEN SEQ QUAL [TAG:TYPE:VALUE ...]; '*' for an absent
//          CIGAR / SEQ / QUAL (qual[0] == 0xff), '=' for RNEXT == RNAME, integer aux types all printed as 'i'.
//   BAM  : "BAM\1", header text, reference dictionary, then block_size-prefixed records whose variable part is the
//          bam1_t::data image as is; 64 KiB BGZF blocks and the 28-byte EOF block.  The bin field is computed from
//          the alignment span (reg2bin); compressed bytes depend on the deflate implementation, the inflated stream
//          does not.
// CRAM needs htslib's codec stack and reference access: Open() fails loudly for it.  BuildIndex() writes <file>.bai for a closed, coordinate-sorted
// BAM: the index is built on the GPU (slx_bam_index_build, include/seqlib_amd_bam.h); false with "Failed to create index" for SAM output, an unsorted file
// or without a GPU.
// UseGpu() before Open() moves the BGZF side of a BAM writer to the GPU (slx_bgzf_*, include/seqlib_amd_bam.h): DEFLATE, CRC32 and framing run there, the
// host serialises records and compresses nothing.  The member cutting is the same, the compressed bytes are the GPU encoder's.  No fallback: without a
// GPU Open() then returns false.  Without UseGpu() the writer is what it was: zlib on the calling thread, no GPU touched.
// SortByCoordinate() after UseGpu() and before Open() makes the file coordinate-sorted (slx_sort_*, include/seqlib_amd_sort.h): WriteHeader() writes the header
// with SO:coordinate, the records of WriteRecord(s) and WriteDevice go into a sorter in HBM in call order, Close() sorts them there -- tid ascending as unsigned,
// then pos, ties in call order -- and writes them; BuildIndex() afterwards succeeds.  Everything must fit the sorter's budget in HBM (half of what is free at
// Open()); what does not is refused by the write that passes it.  No host fallback.  Without SortByCoordinate() the writer behaves exactly as before.
// SortByCoordinate(spill_prefix) is the same for an output beyond that budget: the write that would pass it first writes the sorter's records, sorted, as a run
// file "<spill_prefix>.run%04d.bam" (slx_sort_spill), and Close() merges the runs into the file (slx_merge_*, include/seqlib_amd_merge.h) and removes them; the file
// is byte for byte what the plain overload writes when everything fits.  WriteHeader() comes before the first record, as the runs carry the header.  It does not
// combine with MarkDuplicates(), which works among the records the sorter holds: Open() then returns false with a message.
// MarkDuplicates() after SortByCoordinate() and before Open() makes Close() mark the duplicates among the sorter's records (slx_dup_mark_sorter,
// include/seqlib_amd_dup.h: bit 0x400 rewritten in HBM by that header's rules, the libraries from the header's @RG lines) before they are sorted and written:
// the chain alignToBam, sort, mark, BGZF, BuildIndex() runs with no record on the host.  Without MarkDuplicates() no flag is touched.
// UseGpuSam() before Open() moves a SAM writer's formatting to the GPU (slx_samw_*, include/seqlib_amd_samw.h): WriteRecord(s) serialise the records and hand them
// over, WriteDevice(d, n, d_rec_off, n_records) takes records that lie in HBM -- which is what BWAAligner::alignToBam calls, so that it writes SAM -- and the text
// is byte for byte what the host writer writes (format_sam below is the definition).  With bgzip the text leaves through the GPU BGZF writer as a bgzip'd SAM.
// A record the host writer would also refuse (a reference id outside the header, a cut optional field) fails the call and nothing of that call's records is
// written; B arrays of subtype d, which the host writer prints, are refused here.  No fallback: without a GPU Open() then returns false.  Without UseGpuSam() a
// SAM writer is what it was: format_sam on the calling thread, no GPU touched, WriteDevice refused.
#pragma once
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>
#include <zlib.h>
#include "SeqLib/BamHeader.h"
#include "SeqLib/BamRecord.h"
#include "seqlib_amd_bam.h"
#include "seqlib_amd_sort.h"
#include "seqlib_amd_samw.h"
#include "seqlib_amd_dup.h"

namespace SeqLib {

const int BAM = 4;      // /root/reference/SeqLib/BamWriter.h:10-12
const int SAM = 3;
const int CRAM = 6;

class BamWriter {
public:
    BamWriter() : output_format("wb") {}
    explicit BamWriter(int o)
    {
        switch (o) {
        case BAM: output_format = "wb"; break;
        case CRAM: output_format = "wc"; break;
        case SAM: output_format = "w"; break;
        default: throw std::invalid_argument("Invalid writer type");
        }
    }
    BamWriter(const BamWriter &) = delete;
    BamWriter &operator=(const BamWriter &) = delete;
    ~BamWriter() { Close(); if (marker) slx_dup_free(marker); }

    void SetHeader(const BamHeader &h) { hdr = h; }
    BamHeader Header() const { return hdr; }
    bool IsOpen() const { return fop != nullptr || gz != nullptr || samw != nullptr; }

    // BAM only, before Open(): the BGZF members are compressed on GPU `device` (-1: the current one) instead of by zlib on the calling thread
    bool UseGpu(int device = -1)
    {
        if (IsOpen()) { std::cerr << "BamWriter::UseGpu - call it before Open()" << std::endl; return false; }
        if (output_format != "wb") { std::cerr << "BamWriter::UseGpu - only BAM output is compressed on the GPU" << std::endl; return false; }
        use_gpu = true; gpu_device = device;
        return true;
    }

    // SAM only, before Open(): the lines are formatted on GPU `device` (-1: the current one); bgzip: the file is a bgzip'd SAM, compressed there too
    bool UseGpuSam(int device = -1, bool bgzip = false)
    {
        if (IsOpen()) { std::cerr << "BamWriter::UseGpuSam - call it before Open()" << std::endl; return false; }
        if (output_format != "w") { std::cerr << "BamWriter::UseGpuSam - only SAM output is formatted on the GPU (UseGpu() is for BAM)" << std::endl; return false; }
        use_gpu_sam = true; gpu_device = device; sam_bgzip = bgzip;
        return true;
    }
    bool IsGpuSam() const { return samw != nullptr; }         // an open SAM writer whose lines are formatted on the GPU
    int64_t GpuSamCounter(const char *name) const { return samw ? slx_samw_counter(samw, name) : -1; }          // slx_samw_counter of the open GPU SAM writer

    // after UseGpu(), before Open(): the records are coordinate-sorted in HBM at Close() (see the top of the file)
    bool SortByCoordinate()
    {
        if (IsOpen()) { std::cerr << "BamWriter::SortByCoordinate - call it before Open()" << std::endl; return false; }
        if (output_format != "wb") { std::cerr << "BamWriter::SortByCoordinate - only BAM output is sorted on the GPU" << std::endl; return false; }
        if (!use_gpu) { std::cerr << "BamWriter::SortByCoordinate - the records are sorted on the GPU; call UseGpu() first (no host fallback)" << std::endl; return false; }
        sort_on = true;
        return true;
    }
    // the same, for an output that may pass the sorter's budget: sorted runs go to "<spill_prefix>.run%04d.bam" and Close() merges them (see the top of the file)
    bool SortByCoordinate(const std::string &spill_prefix)
    {
        if (spill_prefix.empty()) { std::cerr << "BamWriter::SortByCoordinate - an empty spill prefix; SortByCoordinate() sorts without run files" << std::endl; return false; }
        if (!SortByCoordinate()) return false;
        spill_prefix_ = spill_prefix;
        return true;
    }
    // after SortByCoordinate(), before Open(): Close() marks the duplicates among the sorter's records before it sorts and writes them (see the top of the file)
    bool MarkDuplicates()
    {
        if (IsOpen()) { std::cerr << "BamWriter::MarkDuplicates - call it before Open()" << std::endl; return false; }
        if (!sort_on) { std::cerr << "BamWriter::MarkDuplicates - duplicates are marked among the sorter's records; call SortByCoordinate() first" << std::endl; return false; }
        mark_on = true;
        return true;
    }
    bool IsMarking() const { return marker != nullptr; }     // an open writer that marks duplicates
    // slx_dup_counter of the marking writer; the counters of the last Close() stay readable until the next Open()
    int64_t MarkCounter(const char *name) const { return marker ? slx_dup_counter(marker, name) : -1; }
    bool IsSorting() const { return sorter != nullptr; }      // an open writer that sorts
    int64_t SortCounter(const char *name) const { return sorter ? slx_sort_counter(sorter, name) : -1; }          // slx_sort_counter of the open sorting writer
    // slx_sort_set of the open sorting writer ("max_bytes", "slab_bytes").  With a budget below four stages of host records a stage shrinks to a quarter of it,
    // so that a spilling writer fills its runs
    bool SortKnob(const char *key, int64_t v)
    {
        if (!sorter) { std::cerr << "BamWriter::SortKnob - no open sorting writer" << std::endl; return false; }
        if (!gpu_ok(slx_sort_set(sorter, key, v))) return false;
        if (!std::strcmp(key, "max_bytes")) sort_stage = std::max<size_t>(1, std::min<size_t>(SORT_STAGE, (size_t)v / 4));
        return true;
    }

    bool Open(const std::string &f)
    {
        if (IsOpen()) return false;                  // don't reopen
        m_out = f;
        if (output_format == "wc") {
            std::cerr << "BamWriter::Open - CRAM output needs htslib; not available in the MI355X drop-in" << std::endl;
            return false;
        }
        if (use_gpu_sam) {
            if (slx_samw_open(f.c_str(), gpu_device, sam_bgzip ? SLX_SAMW_BGZF : 0, &samw) != SLX_OK) {
                std::cerr << "BamWriter::Open - " << slx_last_error() << std::endl;
                samw = nullptr;
                return false;
            }
            return true;
        }
        if (use_gpu) {
            if (mark_on && !spill_prefix_.empty()) {
                std::cerr << "BamWriter::Open - MarkDuplicates() marks among the records the sorter holds and does not combine with SortByCoordinate(spill_prefix); sort with spilling, "
                             "then mark the file (slx_dup_file)" << std::endl;
                return false;
            }
            if (slx_bgzf_open(f.c_str(), gpu_device, &gz) != SLX_OK) {
                std::cerr << "BamWriter::Open - " << slx_last_error() << std::endl;
                gz = nullptr;
                return false;
            }
            if (sort_on && slx_sort_create(gpu_device, &sorter) != SLX_OK) {
                std::cerr << "BamWriter::Open - " << slx_last_error() << std::endl;
                sorter = nullptr;
                (void)slx_bgzf_close(gz); gz = nullptr;
                std::remove(f.c_str());
                return false;
            }
            if (marker) { slx_dup_free(marker); marker = nullptr; }
            if (mark_on && slx_dup_create(gpu_device, &marker) != SLX_OK) {
                std::cerr << "BamWriter::Open - " << slx_last_error() << std::endl;
                marker = nullptr;
                slx_sort_free(sorter); sorter = nullptr;
                (void)slx_bgzf_close(gz); gz = nullptr;
                std::remove(f.c_str());
                return false;
            }
            sort_buf.clear(); sort_off.assign(1, 0);
            sort_stage = SORT_STAGE;
            return true;
        }
        fop = (f == "-") ? stdout : std::fopen(f.c_str(), "wb");
        if (!fop) return false;
        blk.clear();
        return true;
    }

    bool WriteHeader() const
    {
        if (hdr.isEmpty()) {
            std::cerr << "BamWriter::WriteHeader - No header supplied. Provide with SetWriteHeader" << std::endl;
            return false;
        }
        if (!IsOpen()) {
            std::cerr << "BamWriter::WriteHeader - Output not open for writing. Open with Open()" << std::endl;
            return false;
        }
        std::string text = hdr.AsString();
        if (sorter) {                                // SO:coordinate by the rule of slx_sort_header
            std::string so((size_t)slx_sort_header(text.data(), (int64_t)text.size(), nullptr, 0), '\0');
            (void)slx_sort_header(text.data(), (int64_t)text.size(), &so[0], (int64_t)so.size());
            text.swap(so);
        }
        if (samw) {                                  // the names become the RNAME / RNEXT table in HBM
            std::vector<std::string> names;
            std::vector<const char *> ptr;
            for (int i = 0; i < hdr.NumSequences(); ++i) names.push_back(hdr.IDtoName(i));
            for (const std::string &nm : names) ptr.push_back(nm.c_str());
            return gpu_ok(slx_samw_header(samw, text.data(), (int64_t)text.size(), ptr.data(), (int)ptr.size()));
        }
        if (output_format == "w") return std::fwrite(text.data(), 1, text.size(), fop) == text.size();
        std::string h("BAM\1", 4);
        put32(h, (uint32_t)text.size());
        h += text;
        put32(h, (uint32_t)hdr.NumSequences());
        for (int i = 0; i < hdr.NumSequences(); ++i) {
            const std::string nm = hdr.IDtoName(i);
            put32(h, (uint32_t)nm.size() + 1);
            h += nm; h.push_back('\0');
            put32(h, (uint32_t)hdr.GetSequenceLength(i));
        }
        if (sorter && !spill_prefix_.empty() && !gpu_ok(slx_sort_spill(sorter, spill_prefix_.c_str(), h.data(), (int64_t)h.size()))) return false;          // the runs carry the header
        if (gz) return gpu_ok(slx_bgzf_write(gz, h.data(), (int64_t)h.size())) && gpu_ok(slx_bgzf_flush(gz));
        if (!bgzf_write(h.data(), h.size())) return false;
        return bgzf_flush();                         // htslib starts the records in a fresh block
    }

    bool WriteRecord(const BamRecord &r)
    {
        if (!IsOpen()) return false;
        const bam1_t *b = r.raw();
        if (!b) return false;
        if (samw) {
            many.clear();
            put_record(b, many);
            const uint64_t off[2] = {0, many.size()};
            return gpu_ok(slx_samw_write_host(samw, many.data(), (int64_t)many.size(), off, 1));
        }
        if (output_format == "w") {
            std::string line;
            if (!format_sam(b, line)) return false;
            return std::fwrite(line.data(), 1, line.size(), fop) == line.size();
        }
        if (sorter) { put_record(b, sort_buf); sort_off.push_back(sort_buf.size()); return sort_buf.size() < sort_stage || sort_flush(); }
        std::string rec;
        rec.reserve(36 + (size_t)b->l_data);
        put_record(b, rec);
        if (gz) return gpu_ok(slx_bgzf_write(gz, rec.data(), (int64_t)rec.size()));
        return bgzf_write(rec.data(), rec.size());
    }

    // every record of the vector, in order.  Host path: WriteRecord one by one.  GPU path: the records serialised into one reused buffer, one slx_bgzf_write.
    bool WriteRecords(const BamRecordPtrVector &recs)
    {
        if (!IsOpen()) return false;
        if (samw) {                                  // serialised with their offsets into the reused buffers, one slx_samw_write_host
            many.clear(); sort_off.assign(1, 0);
            for (const BamRecordPtr &r : recs) {
                const bam1_t *b = r ? r->raw() : nullptr;
                if (!b) return false;
                put_record(b, many); sort_off.push_back(many.size());
            }
            return gpu_ok(slx_samw_write_host(samw, many.data(), (int64_t)many.size(), sort_off.data(), (int64_t)sort_off.size() - 1));
        }
        if (!gz) {
            for (const BamRecordPtr &r : recs) if (!r || !WriteRecord(*r)) return false;
            return true;
        }
        if (sorter) {                                // serialised with the offsets slx_sort_add_host wants; handed over a stage at a time
            for (const BamRecordPtr &r : recs) {
                const bam1_t *b = r ? r->raw() : nullptr;
                if (!b) return false;
                put_record(b, sort_buf); sort_off.push_back(sort_buf.size());
            }
            return sort_buf.size() < sort_stage || sort_flush();
        }
        many.clear();
        for (const BamRecordPtr &r : recs) {
            const bam1_t *b = r ? r->raw() : nullptr;
            if (!b) return false;
            put_record(b, many);
        }
        return gpu_ok(slx_bgzf_write(gz, many.data(), (int64_t)many.size()));
    }

    // n bytes of block_size-prefixed records that already lie in the HBM of the writer's GPU (slx_rec_build's stream, a reader's slx_bam_batch.d_stream): staged by
    // slx_bgzf_write_device without a host copy; the caller's buffer is free again when the call returns.  Only a BAM writer opened after UseGpu() takes them:
    // false with a message for a SAM writer, a host-zlib writer and a closed writer.
    bool WriteDevice(const void *d, int64_t n)
    {
        if (samw) { std::cerr << "BamWriter::WriteDevice - a GPU SAM writer needs the records' offsets: use WriteDevice(d, n, d_rec_off, n_records)" << std::endl; return false; }
        if (output_format != "wb") { std::cerr << "BamWriter::WriteDevice - only BAM output takes records from the GPU" << std::endl; return false; }
        if (!IsOpen()) { std::cerr << "BamWriter::WriteDevice - Output not open for writing. Open with Open()" << std::endl; return false; }
        if (!gz) { std::cerr << "BamWriter::WriteDevice - the writer compresses on the host; call UseGpu() before Open()" << std::endl; return false; }
        if (sorter) { std::cerr << "BamWriter::WriteDevice - a sorting writer needs the records' offsets: use WriteDevice(d, n, d_rec_off, n_records)" << std::endl; return false; }
        return gpu_ok(slx_bgzf_write_device(gz, d, n));
    }
    // the same with the records' n_records + 1 uint64 offsets in HBM (slx_rec_batch.d_rec_off, slx_bam_batch.d_rec_off): a sorting writer keeps the records in its
    // sorter (slx_sort_add_device), any other GPU writer ignores the offsets and does what WriteDevice(d, n) does
    bool WriteDevice(const void *d, int64_t n, const void *d_rec_off, int64_t n_records)
    {
        if (samw) return gpu_ok(slx_samw_write_device(samw, d, n, d_rec_off, n_records));
        if (!sorter) return WriteDevice(d, n);
        return sort_flush() && gpu_ok(slx_sort_add_device(sorter, d, n, d_rec_off, n_records));          // (what the host wrote before comes before)
    }
    bool IsGpuBam() const { return gz != nullptr; }           // an open BAM writer whose BGZF side runs on the GPU
    int64_t GpuCounter(const char *name) const { return gz ? slx_bgzf_counter(gz, name) : -1; }          // slx_bgzf_counter of the open GPU writer

    bool Close()
    {
        if (samw) {
            const bool ok = gpu_ok(slx_samw_close(samw));    // what is in flight reaches the file; the handle is freed
            samw = nullptr;
            return ok;
        }
        if (gz) {
            bool ok = true;
            if (sorter) {                                    // the sort, and the sorted stream into the writer
                ok = sort_flush();
                if (ok && marker) {
                    const std::string text = hdr.AsString();
                    ok = gpu_ok(slx_dup_set_header(marker, text.data(), (int64_t)text.size())) && gpu_ok(slx_dup_mark_sorter(marker, sorter));
                }
                ok = ok && gpu_ok(slx_sort_finish(sorter, gz));
                slx_sort_free(sorter); sorter = nullptr;
            }
            ok = gpu_ok(slx_bgzf_close(gz)) && ok;           // the last member, the EOF block; the handle is freed
            gz = nullptr;
            return ok;
        }
        if (!fop) return false;
        bool ok = true;
        if (output_format == "wb") {
            ok = bgzf_flush();
            static const unsigned char eof_block[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            ok = std::fwrite(eof_block, 1, 28, fop) == 28 && ok;
        }
        if (fop == stdout) std::fflush(stdout); else ok = std::fclose(fop) == 0 && ok;
        fop = nullptr;
        return ok;
    }

    bool BuildIndex() const
    {
        if (IsOpen()) { std::cerr << "Trying to index open BAM. Close first with Close()" << std::endl; return false; }
        if (m_out.empty()) { std::cerr << "Trying to make index, but no BAM specified" << std::endl; return false; }
        if (output_format != "wb" || m_out == "-" || slx_bam_index_build(m_out.c_str(), -1, nullptr) != SLX_OK) {
            std::cerr << "Failed to create index" << (output_format == "wb" && m_out != "-" ? std::string(": ") + slx_last_error() : std::string()) << std::endl;
            return false;
        }
        return true;
    }
    bool SetCramReference(const std::string &) { return false; }

    friend std::ostream &operator<<(std::ostream &out, const BamWriter &b)
    {
        if (b.IsOpen()) out << "Write format: " << (b.output_format == "w" ? "SAM" : "BAM");
        return out << " Write file " << b.m_out;
    }

    // one SAM text line for a record ('\n'-terminated); false when a reference id is outside the header
    bool format_sam(const bam1_t *b, std::string &o) const
    {
        const bam1_core_t &c = b->core;
        auto rname = [&](int32_t tid, std::string &dst) {
            if (tid < 0) { dst += '*'; return true; }
            if (tid >= hdr.NumSequences()) return false;
            dst += hdr.IDtoName(tid);
            return true;
        };
        o.append(bam_get_qname(b));
        o += '\t'; o += std::to_string(c.flag); o += '\t';
        if (!rname(c.tid, o)) return false;
        o += '\t'; o += std::to_string(c.pos + 1);
        o += '\t'; o += std::to_string((int)c.qual); o += '\t';
        if (c.n_cigar == 0) o += '*';
        else {
            const uint8_t *raw = reinterpret_cast<const uint8_t *>(bam_get_cigar(b));
            for (uint32_t i = 0; i < c.n_cigar; ++i) {
                uint32_t w; std::memcpy(&w, raw + i * 4, 4);
                o += std::to_string(bam_cigar_oplen(w)); o += bam_cigar_opchr(w);
            }
        }
        o += '\t';
        if (c.mtid < 0) o += '*';
        else if (c.mtid == c.tid) o += '=';
        else if (!rname(c.mtid, o)) return false;
        o += '\t'; o += std::to_string(c.mpos + 1);
        o += '\t'; o += std::to_string(c.isize); o += '\t';
        if (c.l_qseq) {
            const uint8_t *s = bam_get_seq(b);
            for (int i = 0; i < c.l_qseq; ++i) o += "=ACMGRSVTWYHKDBN"[bam_seqi(s, i)];
            o += '\t';
            const uint8_t *q = bam_get_qual(b);
            if (q[0] == 0xff) o += '*';
            else for (int i = 0; i < c.l_qseq; ++i) o += (char)(q[i] + 33);
        } else o += "*\t*";
        const uint8_t *s = bam_get_aux(b), *end = b->data + b->l_data;
        while (end - s >= 4) {
            o += '\t'; o += (char)s[0]; o += (char)s[1]; o += ':';
            const uint8_t t = s[2];
            s += 3;
            if (!format_aux(t, s, end, o)) return false;
        }
        o += '\n';
        return true;
    }

private:
    static void put32(std::string &s, uint32_t v) { char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)}; s.append(b, 4); }
    // one BAM record (SAMv1 4.2) appended to rec: block_size, the fixed fields, the bam1_t::data image
    static void put_record(const bam1_t *b, std::string &rec)
    {
        const bam1_core_t &c = b->core;
        put32(rec, (uint32_t)(32 + b->l_data));
        put32(rec, (uint32_t)c.tid);
        put32(rec, (uint32_t)c.pos);
        put32(rec, (uint32_t)reg2bin(c.pos, bam_endpos(b)) << 16 | (uint32_t)c.qual << 8 | (uint32_t)(c.l_qname & 0xff));
        put32(rec, (uint32_t)c.flag << 16 | (uint32_t)(c.n_cigar & 0xffff));
        put32(rec, (uint32_t)c.l_qseq);
        put32(rec, (uint32_t)c.mtid);
        put32(rec, (uint32_t)c.mpos);
        put32(rec, (uint32_t)c.isize);
        rec.append((const char *)b->data, (size_t)b->l_data);
    }
    static bool gpu_ok(int rc)
    {
        if (rc != SLX_OK) std::cerr << "BamWriter - " << slx_last_error() << std::endl;
        return rc == SLX_OK;
    }
    // the records serialised so far into the sorter
    bool sort_flush()
    {
        if (sort_off.size() <= 1) return true;
        const bool ok = gpu_ok(slx_sort_add_host(sorter, sort_buf.data(), (int64_t)sort_buf.size(), sort_off.data(), (int64_t)sort_off.size() - 1));
        sort_buf.clear(); sort_off.assign(1, 0);
        return ok;
    }
    template <typename T> static T rd(const uint8_t *p) { T v; std::memcpy(&v, p, sizeof(T)); return v; }
    static int reg2bin(int64_t beg, int64_t end)     // SAMv1 5.3
    {
        --end;
        if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
        if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
        if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
        if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
        if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
        return 0;
    }
    static bool format_num(uint8_t t, const uint8_t *&s, const uint8_t *end, std::string &o)
    {
        char buf[64];
        switch (t) {
        case 'c': if (end - s < 1) return false; o += std::to_string((int)rd<int8_t>(s)); s += 1; return true;
        case 'C': if (end - s < 1) return false; o += std::to_string((unsigned)rd<uint8_t>(s)); s += 1; return true;
        case 's': if (end - s < 2) return false; o += std::to_string((int)rd<int16_t>(s)); s += 2; return true;
        case 'S': if (end - s < 2) return false; o += std::to_string((unsigned)rd<uint16_t>(s)); s += 2; return true;
        case 'i': if (end - s < 4) return false; o += std::to_string(rd<int32_t>(s)); s += 4; return true;
        case 'I': if (end - s < 4) return false; o += std::to_string(rd<uint32_t>(s)); s += 4; return true;
        case 'f': if (end - s < 4) return false; std::snprintf(buf, sizeof buf, "%g", rd<float>(s)); o += buf; s += 4; return true;
        case 'd': if (end - s < 8) return false; std::snprintf(buf, sizeof buf, "%g", rd<double>(s)); o += buf; s += 8; return true;
        }
        return false;
    }
    static bool format_aux(uint8_t t, const uint8_t *&s, const uint8_t *end, std::string &o)
    {
        switch (t) {
        case 'A': if (end - s < 1) return false; o += "A:"; o += (char)*s++; return true;
        case 'c': case 'C': case 's': case 'S': case 'i': case 'I': o += "i:"; return format_num(t, s, end, o);
        case 'f': o += "f:"; return format_num(t, s, end, o);
        case 'd': o += "d:"; return format_num(t, s, end, o);
        case 'Z': case 'H':
            o += (char)t; o += ':';
            while (s < end && *s) o += (char)*s++;
            if (s >= end) return false;
            ++s;
            return true;
        case 'B': {
            if (end - s < 5) return false;
            const uint8_t sub = *s++;
            const uint32_t n = rd<uint32_t>(s); s += 4;
            o += "B:"; o += (char)sub;
            for (uint32_t i = 0; i < n; ++i) { o += ','; if (!format_num(sub, s, end, o)) return false; }
            return true;
        }
        }
        return false;
    }

    // ---- BGZF (SAMv1 4.1): gzip members of <= 64 KiB carrying their compressed size in a "BC" extra field
    static constexpr size_t BGZF_BLOCK = 0xff00;
    bool bgzf_write(const char *p, size_t n) const
    {
        while (n) {
            const size_t take = std::min(n, BGZF_BLOCK - blk.size());
            blk.append(p, take); p += take; n -= take;
            if (blk.size() == BGZF_BLOCK && !bgzf_flush()) return false;
        }
        return true;
    }
    bool bgzf_flush() const
    {
        if (blk.empty()) return true;
        unsigned char out[0x10000];
        z_stream zs;
        std::memset(&zs, 0, sizeof zs);
        if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
        zs.next_in = (Bytef *)blk.data(); zs.avail_in = (uInt)blk.size();
        zs.next_out = out + 18; zs.avail_out = sizeof out - 18 - 8;
        const int rc = deflate(&zs, Z_FINISH);
        const size_t clen = zs.total_out;
        deflateEnd(&zs);
        if (rc != Z_STREAM_END) return false;
        static const unsigned char head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        std::memcpy(out, head, 16);
        const size_t total = 18 + clen + 8;
        out[16] = (unsigned char)((total - 1) & 0xff); out[17] = (unsigned char)((total - 1) >> 8);
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)blk.data(), (uInt)blk.size());
        const uint32_t isz = (uint32_t)blk.size();
        for (int i = 0; i < 4; ++i) { out[18 + clen + i] = (unsigned char)(crc >> (8 * i)); out[22 + clen + i] = (unsigned char)(isz >> (8 * i)); }
        blk.clear();
        return std::fwrite(out, 1, total, fop) == total;
    }

    std::string m_out;
    std::string output_format;
    FILE *fop = nullptr;
    BamHeader hdr;
    mutable std::string blk;        // uncompressed bytes of the BGZF block being filled
    bool use_gpu = false;           // UseGpu(): the BGZF side runs on the GPU
    int gpu_device = -1;
    slx_bgzf *gz = nullptr;         // the open GPU writer
    std::string many;               // WriteRecords' reused buffer
    bool use_gpu_sam = false;       // UseGpuSam(): the SAM lines are formatted on the GPU
    bool sam_bgzip = false;
    slx_samw *samw = nullptr;       // the open GPU SAM writer
    static constexpr size_t SORT_STAGE = (size_t)16 << 20;          // serialised bytes that make one slx_sort_add_host
    size_t sort_stage = SORT_STAGE;
    bool sort_on = false;           // SortByCoordinate()
    std::string spill_prefix_;      // SortByCoordinate(spill_prefix): where the run files go
    slx_sort *sorter = nullptr;     // of the open sorting writer
    bool mark_on = false;           // MarkDuplicates()
    slx_dup *marker = nullptr;      // of the marking writer; kept after Close() for its counters
    std::string sort_buf;           // records serialised for the sorter, and their offsets
    std::vector<uint64_t> sort_off;
};

}  // namespace SeqLib
