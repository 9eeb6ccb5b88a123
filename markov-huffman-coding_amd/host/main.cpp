// main.cpp — `markovhuffman`, command-line compatible with the reference's driver (src/main.cpp):
//   markov-huffman <input> [-o output] [-h] [-e encoding_file] [-d output_encoding_file] [-g] [-x]
// Same flag grammar (clustered short flags such as -xh; -o/-e/-d take the following arguments in the
// order the letters appear; a bare "-" is accepted; unknown letters only warn), same validation, same
// progress lines on stderr, same file formats.  All per-byte work runs on the GPU through
// coding.h -> libmhc.so.
//
// Extensions use long options the reference's parser never accepted:
//   --index FILE     write (compress) / read (extract) the chunk-index sidecar that lets decode run in
//                    parallel; without it extraction first rebuilds the index on the device
//   --chunk N        symbols per index entry (power of two, 256..8192; default 1024)
//   --device N       HIP device ordinal
//   --range B:E      extract only bytes [B, E) of the original input (repeatable; needs -x and --index)
//   --recode TABLE   with -x, -e and -o: write the stream coded again under TABLE, the decoded bytes never written; with
//                    --index the indexed path, and the output's own index goes to <output>.idx
//   --find STRING    print `pattern begin` per occurrence of STRING in the original input, searched on the device without
//                    decompressing (repeatable, 64 bytes in all; --find-fold folds ASCII case; needs -x and --index)
//   --find-file FILE the same for a dictionary: one pattern per line of FILE (split at LF, empty lines skipped, any other byte
//                    kept; up to 65536 patterns of at most 255 bytes), searched in one pass; not together with --find
//   --redact STRING  with --recode: the occurrences of STRING in the original input are found on the device (repeatable, the
//                    limits of --find; --redact-fold folds ASCII case), merged into spans there, and the stream is coded again
//                    with those bytes replaced by the --mask byte (default 0x2A); the bytes are never written.  The new
//                    table may be the old one.  --redact-file FILE: one pattern per line, the limits of --find-file.
//   --replace STRING with --redact or --redact-file: the occurrences are replaced by STRING (at most 255 bytes; "" deletes
//                    them) instead of being masked, so the output has another length; <output>.idx is written for it
//   --token-key HEX32 with --replace or --replace-file: the 16-byte key (32 hex digits) of keyed tokens.  The first %H of a
//                    replacement string then stands for 16 hex digits of the SipHash-2-4 of the bytes the span matched (under
//                    --redact-fold: of their lower-case form), %NH with N 1..16 for the first N of them; equal matches get equal
//                    tokens (include/mh.h, "TOKENS FROM MATCHED BYTES").  Without the key every string stays literal.
//   --replace-file FILE with --redact-file, not with --replace or --mask: line j of FILE replaces pattern j (split at LF, empty
//                    lines kept: an empty line deletes; a final LF adds no line; as many lines as patterns, at most 255 bytes
//                    each).  Overlapping or touching hits become one span, replaced by the line of its lowest pattern number
//   --crc            with -x: print `crc32 length` of the original input (CRC-32 as zlib computes it, %08x, and the byte
//                    count), taken on the device without decompressing; with --index the indexed path
#include <ctype.h>
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "coding.h"

static void print_help() {
    eprintf("markov-huffman <input> [-o output] [options]\n");
    eprintf("\t-o output_file\n");
    eprintf("\t-h use simple huffman coding\n");
    eprintf("\n");
    eprintf("\t-e encoding_file\n");
    eprintf("\t-d output_encoding_file\n");
    eprintf("\n");
    eprintf("\t-g print huffman trees and tables\n");
    eprintf("\t-x extract\n");
    eprintf("\n");
    eprintf("\t--index file   chunk-index sidecar for parallel extraction (MI355X extension)\n");
    eprintf("\t--chunk n      symbols per index entry (default 1024)\n");
    eprintf("\t--order2       contexts of two previous bytes (MI355X extension; own file formats)\n");
    eprintf("\t--max-code-len n  no code longer than n bits, 8..64 (MI355X extension; when training a table: not with -e, -x, --order2)\n");
    eprintf("\t--device n     HIP device ordinal\n");
    eprintf("\t--range b:e    with -x and --index: extract only bytes [b, e) (repeatable, concatenated in order)\n");
    eprintf("\t--find string  with -x and --index: print `pattern begin` for every occurrence of the string in the original input\n");
    eprintf("\t               without decompressing it (repeatable, 64 bytes in all; --find-fold: ASCII letters match either case);\n");
    eprintf("\t               exit status 0 with hits, 1 with none\n");
    eprintf("\t--find-file f  the same with one pattern per line of `f` (empty lines skipped; at most 255 bytes each), thousands in one\n");
    eprintf("\t               pass; honours --find-fold; not together with --find\n");
    eprintf("\t--crc          with -x: print the CRC-32 (as zlib computes it) and the length of the original input without\n");
    eprintf("\t               decompressing it, as `%%08x %%llu`; with --index the indexed path; no output file is written\n");
    eprintf("\t--recode table with -x, -e and -o: write the stream coded again under `table` (the bytes are never written);\n");
    eprintf("\t               with --index the output's index goes to <output>.idx\n");
    eprintf("\t--redact string  with --recode: every occurrence of the string is replaced by the --mask byte while the stream is coded\n");
    eprintf("\t               again (repeatable, 64 bytes in all; --redact-fold: ASCII letters match either case); `table` may be the -e table\n");
    eprintf("\t--redact-file f  the same with one pattern per line of `f`, as --find-file; not together with --redact\n");
    eprintf("\t--mask byte    the byte that takes the place of redacted bytes: decimal or 0x.., 0 to 255 (default 0x2A)\n");
    eprintf("\t--replace string  with --redact or --redact-file: every occurrence becomes the string (at most 255 bytes, \"\" deletes)\n");
    eprintf("\t--token-key hex32  with --replace or --replace-file: the first %%H (or %%NH, N 1..16) of a replacement stands for 16 (N) hex\n");
    eprintf("\t               digits of the keyed digest of the matched bytes; the key is 32 hex digits\n");
    eprintf("\t--replace-file f  with --redact-file: line j of `f` replaces pattern j (an empty line deletes; where patterns overlap the\n");
    eprintf("\t               earlier line of the pattern file wins); not together with --replace or --mask\n");
    eprintf("\t               instead of mask bytes; not together with --mask\n");
}

struct options {
    bool extract = false, debug = false, simple_huffman = false;
    const char* input = nullptr;
    const char* output = nullptr;
    const char* encoding_input = nullptr;
    const char* encoding_output = nullptr;
    std::string index_path;
    uint32_t chunk = MH_CHUNK_DEFAULT;
    bool order2 = false;
    int max_code_len = 0;                                         // 0: no limit
    int device = -1;
    std::vector<uint64_t> ranges;                                 // begin, end per --range
    std::vector<std::string> finds;                               // one per --find
    bool find_fold = false;
    const char* find_file = nullptr;                              // --find-file: the patterns are its lines, searched as a dictionary
    const char* recode_table = nullptr;                           // --recode: the table the stream is coded again under
    bool crc = false;                                             // --crc: print the digest of the original input
    std::vector<std::string> redacts;                             // one per --redact
    const char* redact_file = nullptr;                            // --redact-file: the patterns are its lines
    bool redact_fold = false, mask_given = false;
    int mask = 0x2A;                                              // --mask: what a redacted byte becomes
    bool replace_given = false;
    std::string replace;                                          // --replace: what a redacted span becomes ("" deletes it)
    const char* replace_file = nullptr;                           // --replace-file: line j replaces pattern j of --redact-file
    std::vector<std::string> replacements;                        // its lines, empty ones kept
    const char* token_key = nullptr;                              // --token-key: %H in a replacement stands for a keyed token
    uint8_t key[16] = {0};
};

// "B:E" with decimal B <= E; anything else is an error
static bool parse_range(const char* v, uint64_t* b, uint64_t* e) {
    const char* colon = strchr(v, ':');
    if (!colon || colon == v || !colon[1] || v[0] == '-' || colon[1] == '-') return false;
    char* end = nullptr;
    errno = 0;
    *b = strtoull(v, &end, 10);
    if (errno || end != colon) return false;
    *e = strtoull(colon + 1, &end, 10);
    if (errno || *end) return false;
    return *b <= *e;
}

// Flag grammar of src/main.cpp:55-101.
static options parse(int argc, char* argv[]) {
    options o;
    for (int i = 1; i < argc; i++) {
        const char* a = argv[i];
        if (a[0] == '-' && a[1] == '-' && a[2] != 0) {           // long options: ours only
            auto need = [&](const char* name) -> const char* {
                if (i + 1 >= argc) { eprintf("Error: Expected a value following %s.\n", name); exit(1); }
                return argv[++i];
            };
            if (!strcmp(a, "--index")) o.index_path = need(a);
            else if (!strcmp(a, "--chunk")) {
                const unsigned long v = strtoul(need(a), nullptr, 10);
                if (v < MH_CHUNK_MIN || v > MH_CHUNK_MAX || (v & (v - 1))) {
                    eprintf("Error: --chunk must be a power of two between %u and %u.\n", MH_CHUNK_MIN, MH_CHUNK_MAX);
                    exit(1);
                }
                o.chunk = (uint32_t)v;
            }
            else if (!strcmp(a, "--device")) o.device = atoi(need(a));
            else if (!strcmp(a, "--order2")) o.order2 = true;
            else if (!strcmp(a, "--max-code-len")) {
                const char* v = need(a);
                char* end = nullptr;
                const long n = strtol(v, &end, 10);
                if (!*v || *end || n < 8 || n > 64) {
                    eprintf("Error: --max-code-len must be between 8 and 64.\n");
                    exit(1);
                }
                o.max_code_len = (int)n;
            }
            else if (!strcmp(a, "--range")) {
                const char* v = need(a);
                uint64_t b = 0, e = 0;
                if (!parse_range(v, &b, &e)) {
                    eprintf("Error: --range expects B:E with B <= E (byte offsets of the original input), got \"%s\".\n", v);
                    exit(1);
                }
                o.ranges.push_back(b);
                o.ranges.push_back(e);
            }
            else if (!strcmp(a, "--find")) o.finds.push_back(need(a));
            else if (!strcmp(a, "--find-file")) o.find_file = need(a);
            else if (!strcmp(a, "--find-fold")) o.find_fold = true;
            else if (!strcmp(a, "--recode")) o.recode_table = need(a);
            else if (!strcmp(a, "--crc")) o.crc = true;
            else if (!strcmp(a, "--redact")) o.redacts.push_back(need(a));
            else if (!strcmp(a, "--redact-file")) o.redact_file = need(a);
            else if (!strcmp(a, "--redact-fold")) o.redact_fold = true;
            else if (!strcmp(a, "--mask")) {
                const char* v = need(a);
                char* end = nullptr;
                errno = 0;
                const unsigned long n = strtoul(v, &end, 0);       // decimal or 0x..
                if (!*v || *end || errno || v[0] == '-' || n > 255) {
                    eprintf("Error: --mask takes a byte value, 0 to 255.\n");
                    exit(1);
                }
                o.mask = (int)n;
                o.mask_given = true;
            }
            else if (!strcmp(a, "--replace")) {
                o.replace = need(a);
                o.replace_given = true;
            }
            else if (!strcmp(a, "--replace-file")) o.replace_file = need(a);
            else if (!strcmp(a, "--token-key")) o.token_key = need(a);
            else eprintf("Warning: Unknown option %s.\n", a);
            continue;
        }
        if (a[0] != '-') {
            if (!o.input) o.input = a;
            else eprintf("Warning: Unexpected positional argument %s.\n", a);
            continue;
        }
        int taken = 0;                                            // following argv entries consumed by this cluster
        for (const char* c = a + 1; *c; ++c) {
            const char** slot = nullptr;
            const char* what = nullptr;
            switch (*c) {
                case 'o': slot = &o.output; what = "output file following -o"; break;
                case 'e': slot = &o.encoding_input; what = "encoding file following -e"; break;
                case 'd': slot = &o.encoding_output; what = "encoding output file following -d"; break;
                case 'x': o.extract = true; break;
                case 'h': o.simple_huffman = true; break;
                case 'g': o.debug = true; break;
                default: eprintf("Warning: Unknown option %c.\n", *c);
            }
            if (slot) {
                if (i + 1 < argc) *slot = argv[i + 1 + taken++];
                else eprintf("Error: Expected %s.\n", what);
            }
        }
        i += taken;
    }
    return o;
}

static FILE* open_or_die(const char* path, const char* mode, const char* what) {
    FILE* f = fopen(path, mode);
    if (!f) {
        eprintf("Error while opening %s; %s.\n", what, strerror(errno));
        exit(1);
    }
    return f;
}

// the patterns of --find-file / --redact-file: the lines of the file, split at LF, empty lines skipped
static void load_patterns(const char* path, const char* flag, std::vector<std::string>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        eprintf("Error: cannot open the %s %s.\n", flag, path);
        exit(1);
    }
    std::string line;
    for (int c; (c = fgetc(f)) != EOF || !line.empty();) {
        if (c != '\n' && c != EOF) { line.push_back((char)c); continue; }
        if (!line.empty()) out.push_back(line);
        line.clear();
        if (c == EOF) break;
    }
    fclose(f);
    if (out.empty()) {
        eprintf("Error: the %s %s holds no pattern.\n", flag, path);
        exit(1);
    }
}

// the replacements of --replace-file: the lines of the file, split at LF, empty lines kept (an empty line deletes); a final
// LF adds no line
static void load_replacements(const char* path, std::vector<std::string>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        eprintf("Error: cannot open the --replace-file %s.\n", path);
        exit(1);
    }
    std::string line;
    bool open_line = false;                                       // bytes, or nothing yet, behind the last LF
    for (int c; (c = fgetc(f)) != EOF;) {
        if (c == '\n') { out.push_back(line); line.clear(); open_line = false; }
        else { line.push_back((char)c); open_line = true; }
    }
    if (open_line) out.push_back(line);
    fclose(f);
}

// the limits of the --find / --redact strings (Shift-And) or of a --find-file / --redact-file (the dictionary)
static void check_patterns(const std::vector<std::string>& pats, bool from_file, const char* flag, const char* file_flag) {
    size_t total = 0;
    for (const std::string& p : pats) total += p.size();
    if (!from_file && total > MH_FIND_MAX_POSITIONS) {
        eprintf("Error: the %s strings are %zu bytes in all; at most %d (%s takes more).\n", flag, total, MH_FIND_MAX_POSITIONS, file_flag);
        exit(1);
    }
    if (from_file) {
        for (const std::string& p : pats)
            if (p.size() > MH_DICT_MAX_LEN) {
                eprintf("Error: a line of the %s is %zu bytes; at most %u.\n", file_flag, p.size(), MH_DICT_MAX_LEN);
                exit(1);
            }
        if (pats.size() > MH_DICT_MAX_PATTERNS) {
            eprintf("Error: the %s holds %zu patterns; at most %u.\n", file_flag, pats.size(), MH_DICT_MAX_PATTERNS);
            exit(1);
        }
    }
}

int main(int argc, char* argv[]) {
    if (argc < 2) {
        print_help();
        return 1;
    }
    options o = parse(argc, argv);
    if (!o.ranges.empty()) {                                       // checked before anything is opened or a device is used
        if (!o.extract || o.index_path.empty()) {
            eprintf("Error: --range needs -x and --index.\n");
            exit(1);
        }
        if (o.order2) {
            eprintf("Error: --range does not support --order2.\n");
            exit(1);
        }
    }

    if (o.find_file) {                                             // its lines take the place of the --find strings
        if (!o.finds.empty()) {
            eprintf("Error: --find-file cannot be combined with --find.\n");
            exit(1);
        }
        load_patterns(o.find_file, "--find-file", o.finds);
    }
    if (o.find_fold && o.finds.empty()) {
        eprintf("Error: --find-fold needs --find.\n");
        exit(1);
    }
    if (!o.finds.empty()) {                                        // the same rules as --range, checked as early
        if (!o.extract || o.index_path.empty()) {
            eprintf("Error: --find needs -x and --index.\n");
            exit(1);
        }
        if (o.order2) {
            eprintf("Error: --find does not support --order2.\n");
            exit(1);
        }
        if (!o.ranges.empty()) {
            eprintf("Error: --find cannot be combined with --range.\n");
            exit(1);
        }
        for (const std::string& p : o.finds)
            if (p.empty()) {
                eprintf("Error: --find expects a non-empty string.\n");
                exit(1);
            }
        check_patterns(o.finds, o.find_file != nullptr, "--find", "--find-file");
    }

    if (o.recode_table) {                                          // checked before anything is opened or a device is used
        if (!o.extract || !o.encoding_input || !o.output) {
            eprintf("Error: --recode needs -x, -e and -o.\n");
            exit(1);
        }
        if (!o.finds.empty() || !o.ranges.empty()) {
            eprintf("Error: --recode cannot be combined with --find or --range.\n");
            exit(1);
        }
        if (o.order2) {
            eprintf("Error: --recode does not support --order2.\n");
            exit(1);
        }
    }
    const bool redact = !o.redacts.empty() || o.redact_file;
    if (o.replace_given) {
        if (!redact) {
            eprintf("Error: --replace needs --redact or --redact-file.\n");
            exit(1);
        }
        if (o.mask_given) {
            eprintf("Error: --replace and --mask cannot be combined.\n");
            exit(1);
        }
        if (o.replace.size() > MH_SPLICE_MAX_REP) {
            eprintf("Error: --replace takes at most %u bytes.\n", MH_SPLICE_MAX_REP);
            exit(1);
        }
    }
    if (o.replace_file) {
        if (!o.redact_file) {
            eprintf("Error: --replace-file needs --redact-file.\n");
            exit(1);
        }
        if (o.replace_given || o.mask_given) {
            eprintf("Error: --replace-file cannot be combined with --replace or --mask.\n");
            exit(1);
        }
    }
    if (o.token_key) {
        if (!o.replace_given && !o.replace_file) {
            eprintf("Error: --token-key needs --replace or --replace-file.\n");
            exit(1);
        }
        bool ok = strlen(o.token_key) == 32;
        for (int k = 0; ok && k < 32; ++k) ok = isxdigit((unsigned char)o.token_key[k]) != 0;
        if (!ok) {
            eprintf("Error: --token-key takes 32 hex digits.\n");
            exit(1);
        }
        for (int k = 0; k < 16; ++k) {
            const char two[3] = {o.token_key[2 * k], o.token_key[2 * k + 1], 0};
            o.key[k] = (uint8_t)strtoul(two, nullptr, 16);
        }
        token_format f;
        if (o.replace_given && !parse_token_format(o.replace, f)) {
            eprintf("Error: --replace takes at most %u bytes, the token's digits included.\n", MH_SPLICE_MAX_REP);
            exit(1);
        }
    }
    if (redact) {                                                  // the rules first, then the pattern file, then everything else
        if (!o.recode_table) {
            eprintf("Error: --redact needs --recode.\n");
            exit(1);
        }
        if (!o.redacts.empty() && o.redact_file) {
            eprintf("Error: --redact and --redact-file cannot be combined.\n");
            exit(1);
        }
        for (const std::string& p : o.redacts)
            if (p.empty()) {
                eprintf("Error: --redact takes a non-empty string.\n");
                exit(1);
            }
        if (o.redact_file) load_patterns(o.redact_file, "--redact-file", o.redacts);
        check_patterns(o.redacts, o.redact_file != nullptr, "--redact", "--redact-file");
        if (o.replace_file) {
            load_replacements(o.replace_file, o.replacements);
            if (o.replacements.size() != o.redacts.size()) {
                eprintf("Error: the --replace-file %s holds %zu lines for %zu patterns.\n", o.replace_file, o.replacements.size(), o.redacts.size());
                exit(1);
            }
            for (const std::string& r : o.replacements)
                if (r.size() > MH_SPLICE_MAX_REP) {
                    eprintf("Error: a line of the --replace-file takes at most %u bytes.\n", MH_SPLICE_MAX_REP);
                    exit(1);
                }
            token_format f;
            for (const std::string& r : o.replacements)
                if (o.token_key && !parse_token_format(r, f)) {
                    eprintf("Error: a line of the --replace-file takes at most %u bytes, the token's digits included.\n", MH_SPLICE_MAX_REP);
                    exit(1);
                }
        }
    } else if (o.mask_given || o.redact_fold) {
        eprintf("Error: --mask and --redact-fold need --redact or --redact-file.\n");
        exit(1);
    }

    if (o.crc) {                                                   // checked before anything is opened or a device is used
        if (!o.extract) {
            eprintf("Error: --crc needs -x.\n");
            exit(1);
        }
        if (!o.finds.empty() || !o.ranges.empty() || o.recode_table) {
            eprintf("Error: --crc cannot be combined with --find, --range or --recode.\n");
            exit(1);
        }
        if (o.order2) {
            eprintf("Error: --crc does not support --order2.\n");
            exit(1);
        }
    }

    if (o.max_code_len && (o.encoding_input || o.extract || o.order2)) {
        eprintf("Error: --max-code-len limits a table that is being trained; it cannot be combined with -e, -x or --order2.\n");
        exit(1);
    }

    // validation of src/main.cpp:103-115
    if (!o.input) {
        eprintf("Error: Must provide input file.\n");
        exit(1);
    }
    if (o.encoding_input && o.encoding_output) {
        eprintf("Error: Don't provide an encoding input and an encoding output. Just use cp.\n");
        exit(1);
    }
    if (o.extract && !o.encoding_input) {
        eprintf("Error: Must provide encoding file input while in decompress mode.\n");
        exit(1);
    }
    if (mh_device_count() < 1) {
        eprintf("Error: no usable HIP device; this build has no CPU path.\n");
        exit(1);
    }
    if (o.device >= 0) mh_or_die(mh_set_device(o.device), "--device");

    check_access(o.input, false);                                  // src/main.cpp:118-121 (prints only)
    if (o.output) check_access(o.output, true);
    if (o.encoding_input) check_access(o.encoding_input, false);
    if (o.encoding_output) check_access(o.encoding_output, false);

    FILE* input_fd = open_or_die(o.input, "rb", "input");
    FILE* output_fd = o.output && o.finds.empty() && !o.crc ? open_or_die(o.output, "w+b", "output") : stdout;   // read-write: the result is written through a mapping

    i_coding_provider* coder = nullptr;
    if (o.encoding_input) {
        eprintf("Loading encoding table from file...\n");
        FILE* fd = open_or_die(o.encoding_input, "rb", "encoding input");
        bitbuffer buffer(fd, bitbuffer::read);
        if (o.order2) {
            coder = new markov2_huffman_table(buffer);             // its loader checks the order-2 header
        } else
        // first bit: 0 = Huffman tree, 1 = Markov-Huffman file (src/main.cpp:147-161)
        if (buffer.peek_bit() != !o.simple_huffman) {
            eprintf("Error: Incorrect encoding table provided for current operation; expected %s, found %s.\n",
                    o.simple_huffman ? "simple Huffman" : "Markov-Huffman",
                    buffer.peek_bit() ? "Markov-Huffman" : "simple Huffman");
            exit(1);
        }
        if (coder) {}
        else if (buffer.peek_bit() == 0) coder = new huffman_table(buffer);
        else coder = new markov_huffman_table(buffer);
    } else {
        std::vector<uint64_t> counts(o.order2 ? (size_t(1) << 24) : o.simple_huffman ? 256 : 65536);
        if (o.order2) {
            eprintf("Building order-2 Markov-Huffman encoding table from input...\n");
            construct_table(input_fd, 2, counts.data());
            coder = new markov2_huffman_table(counts.data());
        } else if (o.simple_huffman) {
            eprintf("Building simple Huffman encoding table from input...\n");
            construct_table(input_fd, 0, counts.data());
            coder = new huffman_table(counts.data(), o.max_code_len);
        } else {
            eprintf("Building Markov-Huffman encoding table from input...\n");
            construct_table(input_fd, 1, counts.data());
            coder = new markov_huffman_table(counts.data(), o.max_code_len);
        }
        fseek(input_fd, 0, SEEK_SET);                              // src/main.cpp:183
    }
    if (!o.index_path.empty()) coder->set_index_path(o.index_path, o.chunk);
    if (!o.ranges.empty()) coder->set_ranges(o.ranges);

    if (o.debug) {                                                 // src/main.cpp:186-190
        coder->print_table();
        coder->print_tree();
    }

    if (o.encoding_output) {                                       // src/main.cpp:192-202
        FILE* fd = fopen(o.encoding_output, "wb");
        eprintf("Writing encoding table to %s...\n", o.encoding_output);
        if (!fd) {
            eprintf("Error while opening encoding file output; %s.\n", strerror(errno));
            exit(1);
        }
        bitbuffer buffer(fd, bitbuffer::write);
        coder->write_coding_tree(buffer);
    }

    if (!o.finds.empty()) {                                        // prints the hits; no output file
        eprintf("Searching %s...\n", o.input);
        const uint64_t hits = coder->find(input_fd, o.finds, o.find_fold, o.find_file != nullptr);
        delete coder;
        eprintf("Done.\n");
        return hits ? 0 : 1;
    }
    if (o.crc) {                                                   // prints the digest; no output file
        eprintf("Checksumming %s...\n", o.input);
        coder->crc(input_fd);
        delete coder;
        eprintf("Done.\n");
        return 0;
    }
    if (o.recode_table) {                                          // the new table: either kind, whatever the old one is
        FILE* fd = open_or_die(o.recode_table, "rb", "--recode table");
        bitbuffer buffer(fd, bitbuffer::read);
        {                                                          // an order-2 table: refused by name, not by the loader's type error
            std::vector<uint8_t> bytes;
            FILE* tf = open_or_die(o.recode_table, "rb", "--recode table");
            uint8_t chunk[65536];
            for (size_t k; (k = fread(chunk, 1, sizeof chunk, tf)) > 0;) bytes.insert(bytes.end(), chunk, chunk + k);
            fclose(tf);
            mh_model* probe = nullptr;
            if (mh_model_from_table_bits(bytes.data(), bytes.size(), &probe) == MH_OK && mh_model_type(probe) == 2) {
                eprintf("Error: --recode does not support an order-2 table (%s).\n", o.recode_table);
                exit(1);
            }
            mh_model_free(probe);
        }
        i_coding_provider* dst = buffer.peek_bit() == 0 ? (i_coding_provider*)new huffman_table(buffer) : new markov_huffman_table(buffer);
        eprintf("Re-coding %s ===> %s...\n", o.input, o.output);
        redact_options ro;
        ro.patterns = o.redacts;
        ro.fold = o.redact_fold;
        ro.dict = o.redact_file != nullptr;
        ro.mask = (uint8_t)o.mask;
        ro.replace = o.replace_given;
        ro.rep = o.replace;
        ro.table = o.replace_file != nullptr;
        ro.reps = o.replacements;
        ro.token = o.token_key != nullptr;
        memcpy(ro.key, o.key, 16);
        coder->recode(input_fd, output_fd, *dst, std::string(o.output) + ".idx", redact ? &ro : nullptr);
        delete dst;
        delete coder;
        eprintf("Done.\n");
        return 0;
    }
    if (o.extract) {
        eprintf("Extracting %s ===> %s...\n", o.input, o.output);
        coder->decompress(input_fd, output_fd);
    } else {
        eprintf("Compressing %s ===> %s...\n", o.input, o.output);
        coder->compress(input_fd, output_fd);
    }
    delete coder;
    eprintf("Done.\n");
    return 0;
}
