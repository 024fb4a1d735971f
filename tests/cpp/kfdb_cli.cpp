// kfdb_cli -- drives orbx::ORBVocabulary / orbx::KeyFrameDatabase (include/orbx.hpp) from a
// script, for tests/test_kfdb_cpp.py.
//
//   kfdb_cli <vocabulary.txt | -> <script> <max_keyframes> <max_words>
//
// Script lines (a BowVector is "n w0 v0 w1 v1 ...", values as %.17g):
//   score <bow> <bow>            -> "score <hex bits of the double>"  (needs no vocabulary)
//   add <id> <bow>
//   erase <id>
//   clear
//   covis <id> <n> <ids...>
//   reloc <bow>                  -> "cand <ids...>"
//   loop <min_score %.9g> <n> <connected ids...> <bow>   -> "cand <ids...>"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <set>
#include <sstream>
#include <string>

#include "orbx.hpp"

static orbx::BowVector read_bow(std::istringstream& in) {
    int n = 0;
    in >> n;
    orbx::BowVector v;
    for (int i = 0; i < n; i++) {
        int32_t w;
        std::string s;
        in >> w >> s;
        v[w] = std::strtod(s.c_str(), nullptr);
    }
    return v;
}

static void print_cand(const std::vector<int32_t>& c) {
    std::printf("cand");
    for (int32_t id : c) std::printf(" %d", id);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: kfdb_cli <vocabulary.txt|-> <script> <max_keyframes> <max_words>\n");
        return 2;
    }
    try {
        std::unique_ptr<orbx::ORBVocabulary> voc;
        std::unique_ptr<orbx::KeyFrameDatabase> db;
        if (std::strcmp(argv[1], "-") != 0) {
            voc.reset(new orbx::ORBVocabulary(0));
            if (!voc->loadFromTextFile(argv[1])) {
                std::fprintf(stderr, "vocabulary rejected\n");
                return 1;
            }
            db.reset(new orbx::KeyFrameDatabase(*voc, std::atoi(argv[3]), std::atoi(argv[4])));
        }
        std::ifstream script(argv[2]);
        std::string line;
        while (std::getline(script, line)) {
            std::istringstream in(line);
            std::string op;
            if (!(in >> op)) continue;
            if (op == "score") {
                const orbx::BowVector a = read_bow(in), b = read_bow(in);
                const double s = orbx::BowScore(a, b);
                uint64_t bits;
                std::memcpy(&bits, &s, 8);
                std::printf("score %016" PRIx64 "\n", bits);
                continue;
            }
            if (!db) {
                std::fprintf(stderr, "'%s' needs a vocabulary\n", op.c_str());
                return 1;
            }
            if (op == "add") {
                int id;
                in >> id;
                db->add(id, read_bow(in));
            } else if (op == "erase") {
                int id;
                in >> id;
                db->erase(id);
            } else if (op == "clear") {
                db->clear();
            } else if (op == "covis") {
                int id, n;
                in >> id >> n;
                std::vector<int32_t> best((size_t)n);
                for (auto& b : best) in >> b;
                db->SetBestCovisibility(id, best);
            } else if (op == "reloc") {
                print_cand(db->DetectRelocalizationCandidates(read_bow(in)));
            } else if (op == "loop") {
                std::string ms;
                int n;
                in >> ms >> n;
                std::set<int32_t> conn;
                for (int i = 0; i < n; i++) {
                    int32_t c;
                    in >> c;
                    conn.insert(c);
                }
                print_cand(db->DetectLoopCandidates(read_bow(in), conn, std::strtof(ms.c_str(), nullptr)));
            } else {
                std::fprintf(stderr, "unknown op '%s'\n", op.c_str());
                return 1;
            }
        }
    } catch (const orbx::Error& e) {
        std::fprintf(stderr, "%s (code %d)\n", e.what(), e.code);
        return 1;
    }
    return 0;
}
