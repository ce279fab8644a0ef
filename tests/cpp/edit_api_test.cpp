// SeqLib::RecordEditor, RefGenome::WriteNmMd and the host calls BamRecord gained with them, through the headers only (tests/test_cpp_edit.py builds and runs it).
//   edit_api_test host                                  no GPU: RemoveTag, RemoveAllTags, ClearSeqQualAndTags, GetFloatTag against hand-written bytes; the plan's
//                                                       refusals as std::invalid_argument
//   edit_api_test hostloop <records.bin> <out.bin>      no GPU: the host loop's edits (RemoveTag / AddZTag / AddIntTag) over a stream of records, for Python to compare
//   edit_api_test edit <in.bam> <gpu.bam> <host.bam> <how>      GPU: BamReader -> RecordEditor -> BamWriter(UseGpu) into <gpu.bam>, and the host loop Next() + RemoveTag /
//                                                       AddZTag / AddIntTag + WriteRecord into <host.bam>; <how> is all, regions or filter (mapq >= 30)
//   edit_api_test calmd <fa> <in.bam> <gpu.bam> <host.bam>      GPU: RefGenome::WriteNmMd into <gpu.bam>; NmMd + host AddIntTag / AddZTag into <host.bam>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/BamRecord.h"
#include "SeqLib/BamWriter.h"
#include "SeqLib/ReadFilter.h"
#include "SeqLib/RecordEditor.h"
#include "SeqLib/RefGenome.h"

using namespace SeqLib;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static BamRecordPtr record_with(const std::string &aux)
{
    const std::string name = "rec";
    const int len = 5;
    BamRecordPtr r = std::make_shared<BamRecord>();
    bam1_t *b = r->raw();
    b->core.tid = 0; b->core.pos = 7; b->core.qual = 30; b->core.n_cigar = 1; b->core.mtid = -1; b->core.mpos = -1;
    b->core.l_qname = (uint16_t)(name.size() + 1); b->core.l_qseq = len;
    const size_t fixed = b->core.l_qname + 4 + (size_t)(len + 1) / 2 + (size_t)len;
    b->l_data = (int)(fixed + aux.size());
    b->data = (uint8_t *)std::calloc((size_t)b->l_data, 1);
    b->m_data = (uint32_t)b->l_data;
    std::memcpy(b->data, name.c_str(), name.size() + 1);
    const uint32_t w = (uint32_t)len << 4;
    std::memcpy(b->data + b->core.l_qname, &w, 4);
    std::memset(b->data + b->core.l_qname + 4, 0x12, (size_t)(len + 1) / 2);
    std::memset(b->data + b->core.l_qname + 4 + (len + 1) / 2, 30, (size_t)len);
    std::memcpy(b->data + fixed, aux.data(), aux.size());
    return r;
}
static std::string aux_of(const BamRecord &r)
{
    const bam1_t *b = r.raw();
    const uint8_t *a = bam_get_aux(b);
    return std::string((const char *)a, (size_t)(b->data + b->l_data - a));
}

static int host()
{
    const float f = 1.5f;
    const double d = -2.25;
    std::string ftag("XFf"), dtag("XDd");
    ftag.append((const char *)&f, 4); dtag.append((const char *)&d, 8);
    const std::string xa1("XAZfirst;\0", 10), nm("NMi\x05\0\0\0", 7), xa2("XAZsecond;\0", 11), rg("RGZgrp\0", 7);
    BamRecordPtr r = record_with(xa1 + nm + ftag + xa2 + dtag + rg);
    float v = 0;
    CHECK(r->GetFloatTag("XF", v) && v == 1.5f);
    CHECK(r->GetFloatTag("XD", v) && v == -2.25f);
    CHECK(!r->GetFloatTag("NM", v) && !r->GetFloatTag("ZZ", v) && !r->GetFloatTag("RG", v));
    r->RemoveTag("ZZ");                                           // absent: nothing
    CHECK(aux_of(*r) == xa1 + nm + ftag + xa2 + dtag + rg);
    r->RemoveTag("XA");                                           // the first occurrence only
    CHECK(aux_of(*r) == nm + ftag + xa2 + dtag + rg);
    r->RemoveTag("RG");                                           // the last field
    CHECK(aux_of(*r) == nm + ftag + xa2 + dtag);
    r->RemoveTag("XA");
    CHECK(aux_of(*r) == nm + ftag + dtag);
    r->AddZTag("RG", "new");
    CHECK(aux_of(*r) == nm + ftag + dtag + std::string("RGZnew\0", 7));
    const int before = r->raw()->l_data;
    r->RemoveAllTags();
    CHECK(aux_of(*r).empty() && r->raw()->l_data == before - (int)(nm.size() + ftag.size() + dtag.size() + 7) && r->Length() == 5 && r->Sequence() == "ACACA");
    r->AddIntTag("XN", 9);
    CHECK(aux_of(*r) == std::string("XNi\x09\0\0\0", 7));
    r->ClearSeqQualAndTags();
    CHECK(r->Length() == 0 && r->raw()->l_data == 4 + 4 && r->Qname() == "rec" && r->CigarString() == "5M" && aux_of(*r).empty() && r->Sequence().empty());
    r->AddZTag("RG", "x");
    CHECK(aux_of(*r) == std::string("RGZx\0", 5));
    // the plan's refusals, on a host-only editor
    RecordEditor ed(SLX_EDIT_HOST);
    int refused = 0;
    auto bad = [&](auto call) { try { call(); } catch (const std::invalid_argument &) { ++refused; } };
    bad([&] { ed.DropTag("X"); }); bad([&] { ed.DropTag("1A"); }); bad([&] { ed.AddZTag("RG", ""); }); bad([&] { ed.AddZTag("RG", std::string("a\0b", 3)); });
    ed.AddIntTag("NM", 1);
    bad([&] { ed.AddZTag("NM", "x"); }); bad([&] { ed.AddIntTag("NM", 2, true); });
    CHECK(refused == 6);
    bool threw = false;
    try { ed.Apply(nullptr, 0, nullptr, 0); } catch (const std::runtime_error &e) { threw = std::strstr(e.what(), "edited on MI355X only") != nullptr; }
    CHECK(threw);
    std::printf("edit api host OK\n");
    return 0;
}

// the host loop's edits over a stream of block_size-prefixed records in a file, no reader and no GPU: what `edit` compares the GPU with, held against Python here
static int hostloop(const std::string &in, const std::string &out)
{
    FILE *f = std::fopen(in.c_str(), "rb");
    CHECK(f);
    std::vector<uint8_t> s;
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) s.insert(s.end(), buf, buf + got);
    std::fclose(f);
    FILE *o = std::fopen(out.c_str(), "wb");
    CHECK(o);
    size_t n = 0;
    for (size_t at = 0; at + 36 <= s.size(); ++n) {
        uint32_t bs; std::memcpy(&bs, &s[at], 4);
        BamRecord r;
        bam1_t *b = r.raw();
        const uint8_t *p = &s[at];
        uint16_t u16; int32_t i32;
        std::memcpy(&i32, p + 4, 4); b->core.tid = i32; std::memcpy(&i32, p + 8, 4); b->core.pos = i32;
        b->core.l_qname = p[12]; b->core.qual = p[13];
        std::memcpy(&u16, p + 14, 2); b->core.bin = u16; std::memcpy(&u16, p + 16, 2); b->core.n_cigar = u16; std::memcpy(&u16, p + 18, 2); b->core.flag = u16;
        std::memcpy(&i32, p + 20, 4); b->core.l_qseq = i32; std::memcpy(&i32, p + 24, 4); b->core.mtid = i32; std::memcpy(&i32, p + 28, 4); b->core.mpos = i32;
        std::memcpy(&i32, p + 32, 4); b->core.isize = i32;
        b->l_data = (int)bs - 32; b->m_data = (uint32_t)b->l_data;
        b->data = (uint8_t *)std::malloc((size_t)b->l_data + 1);
        std::memcpy(b->data, p + 36, (size_t)b->l_data);
        r.RemoveTag("XA"); r.RemoveTag("SA");
        r.AddZTag("RG", "grp1"); r.AddIntTag("XN", 7);
        r.RemoveTag("NM"); r.AddIntTag("NM", 3);
        const std::vector<uint8_t> packed = detail::packed_record(b);
        CHECK(std::fwrite(packed.data(), 1, packed.size(), o) == packed.size());
        at += 4 + (size_t)bs;
    }
    std::fclose(o);
    std::printf("edit api hostloop OK %zu\n", n);
    return 0;
}

static bool restrict_reader(BamReader &rd, const std::string &how, Filter::ReadFilterCollection &fc)
{
    if (how == "regions") {
        GRC grc;
        grc.add(GenomicRegion(0, 1000, 9000)); grc.add(GenomicRegion(1, 0, 2000)); grc.add(GenomicRegion(0, 8000, 20000));
        return rd.SetRegions(grc);
    }
    if (how == "filter") {
        Filter::AbstractRule q;
        q.mapq = Filter::Range(30, 255, false);
        Filter::ReadFilter f;
        f.AddRule(q);
        fc.AddReadFilter(f);
        return rd.SetReadFilter(fc);
    }
    return true;
}

static int edit(const std::string &in, const std::string &gpu_out, const std::string &host_out, const std::string &how)
{
    size_t n_gpu = 0, n_host = 0;
    {
        BamReader rd;
        CHECK(rd.Open(in));
        rd.SetBatchBytes(6000);
        Filter::ReadFilterCollection fc;
        CHECK(restrict_reader(rd, how, fc));
        BamWriter w;
        w.SetHeader(rd.Header());
        CHECK(w.UseGpu() && w.Open(gpu_out) && w.WriteHeader());
        RecordEditor ed;
        ed.DropTag("XA"); ed.DropTag("SA");
        ed.AddZTag("RG", "grp1"); ed.AddIntTag("XN", 7); ed.AddIntTag("NM", 3, true);
        for (int k = 0; k < 2; ++k) {          // two records of the first batch by hand: Apply then takes the rest of that batch
            std::optional<BamRecord> r = rd.Next();
            CHECK(r.has_value());
            r->RemoveTag("XA"); r->RemoveTag("SA");
            r->AddZTag("RG", "grp1"); r->AddIntTag("XN", 7);
            r->RemoveTag("NM"); r->AddIntTag("NM", 3);
            CHECK(w.WriteRecord(*r));
            ++n_gpu;
        }
        while (ed.Apply(rd)) {
            const slx_edit_batch &b = ed.Batch();
            CHECK(w.WriteDevice(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records));
            n_gpu += (size_t)b.n_records;
        }
        CHECK(w.Close() && ed.Counter("us_gather") >= 0);
    }
    {
        BamReader rd;
        CHECK(rd.Open(in));
        rd.SetBatchBytes(6000);
        Filter::ReadFilterCollection fc;
        CHECK(restrict_reader(rd, how, fc));
        BamWriter w;
        w.SetHeader(rd.Header());
        CHECK(w.Open(host_out) && w.WriteHeader());
        while (std::optional<BamRecord> r = rd.Next()) {
            r->RemoveTag("XA"); r->RemoveTag("SA");
            r->AddZTag("RG", "grp1"); r->AddIntTag("XN", 7);
            r->RemoveTag("NM"); r->AddIntTag("NM", 3);
            CHECK(w.WriteRecord(*r));
            ++n_host;
        }
        CHECK(w.Close());
    }
    CHECK(n_gpu == n_host);
    std::printf("edit api edit OK %zu\n", n_gpu);
    return 0;
}

static int calmd(const std::string &fa, const std::string &in, const std::string &gpu_out, const std::string &host_out)
{
    RefGenome ref;
    CHECK(ref.LoadIndex(fa));
    size_t n_gpu = 0, n_host = 0;
    {
        BamReader rd;
        CHECK(rd.Open(in));
        rd.SetBatchBytes(6000);
        BamWriter w;
        w.SetHeader(rd.Header());
        CHECK(w.UseGpu() && w.Open(gpu_out) && w.WriteHeader());
        RecordEditor ed;
        ed.DropTag("XA");
        while (size_t k = ref.WriteNmMd(rd, ed)) {
            const slx_edit_batch &b = ed.Batch();
            CHECK((size_t)b.n_records == k && w.WriteDevice(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records));
            n_gpu += k;
        }
        CHECK(w.Close());
        // the two column adds were the calls' own: the editor is what the caller made it, and a plain Apply goes through
        BamReader again;
        CHECK(again.Open(in));
        again.SetBatchBytes(6000);
        CHECK(ed.Apply(again) && ed.Batch().n_records > 0);
        // a plan without room for the two adds, or with an NM add of its own: std::invalid_argument, and the plan stays as it was
        RecordEditor full;
        for (int k = 0; k < 7; ++k) full.AddIntTag("A" + std::to_string(k), k);
        RecordEditor own;
        own.AddIntTag("NM", 0);
        int refused = 0;
        try { ref.WriteNmMd(again, full); } catch (const std::invalid_argument &) { ++refused; }
        try { ref.WriteNmMd(again, own); } catch (const std::invalid_argument &) { ++refused; }
        CHECK(refused == 2);
        full.AddIntTag("A7", 7);          // (the eighth add still fits: the refused call left nothing behind)
    }
    {
        BamReader rd, rd2;
        CHECK(rd.Open(in) && rd2.Open(in));
        rd.SetBatchBytes(6000); rd2.SetBatchBytes(6000);
        BamWriter w;
        w.SetHeader(rd.Header());
        CHECK(w.Open(host_out) && w.WriteHeader());
        std::vector<int32_t> nm;
        std::vector<std::string> md;
        while (size_t k = ref.NmMd(rd, nm, md)) {
            for (size_t i = 0; i < k; ++i) {
                std::optional<BamRecord> r = rd2.Next();
                CHECK(r.has_value());
                r->RemoveTag("XA");
                if (nm[i] >= 0) { r->RemoveTag("NM"); r->AddIntTag("NM", nm[i]); }
                r->AddZTag("MD", md[i]);
                CHECK(w.WriteRecord(*r));
                ++n_host;
            }
        }
        CHECK(w.Close());
    }
    CHECK(n_gpu == n_host);
    std::printf("edit api calmd OK %zu\n", n_gpu);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 2 && !std::strcmp(argv[1], "host")) return host();
        if (argc == 4 && !std::strcmp(argv[1], "hostloop")) return hostloop(argv[2], argv[3]);
        if (argc == 6 && !std::strcmp(argv[1], "edit")) return edit(argv[2], argv[3], argv[4], argv[5]);
        if (argc == 6 && !std::strcmp(argv[1], "calmd")) return calmd(argv[2], argv[3], argv[4], argv[5]);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    return 2;
}
