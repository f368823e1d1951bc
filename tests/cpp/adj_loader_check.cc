// adj_loader_check.cc -- gm_graph::load_adjacency_list, the node keys, GM_Reader and GM_Tokenizer, dumped as text for
// tests/test_bc_adj_host.py:
//     adj_loader_check <file.adj> <vertex schema> <edge schema> <dump>      (a schema: one of b i l f d per value, or -)
// With -DADJ_CHECK_STUBS the device calls gm_graph.cc refers to are defined here, so that the host sources can be
// compiled into one stand-alone program (the sanitizer build) without the device library.
#include <stdio.h>
#include <string.h>

#include <string>

#include "gm.h"
#include "gm_file_handling.h"
#include "gm_util.h"

#ifdef ADJ_CHECK_STUBS
extern "C" {   // (C linkage: only the names matter; every call reports failure, which sends gm_graph to its host paths)
int gmx_graph_upload() { return -2; }
int gmx_graph_download() { return -2; }
int gmx_graph_free() { return 0; }
int gmx_graph_create_rmat() { return -2; }
int gmx_graph_edge_order() { return -2; }
int gmx_graph_reverse_edge_map() { return -2; }
int gmx_device_count() { return -2; }
long gmx_graph_num_nodes() { return -1; }
long gmx_graph_num_edges() { return -1; }
const char* gmx_last_error() { return "no device in this build"; }
}
#endif

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            printf("%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                \
        }                                                            \
    } while (0)

static bool schema_of(const char* s, std::vector<VALUE_TYPE>& out) {
    for (; *s && *s != '-'; s++) {
        switch (*s) {
            case 'b': out.push_back(GMTYPE_BOOL); break;
            case 'i': out.push_back(GMTYPE_INT); break;
            case 'l': out.push_back(GMTYPE_LONG); break;
            case 'f': out.push_back(GMTYPE_FLOAT); break;
            case 'd': out.push_back(GMTYPE_DOUBLE); break;
            default: return false;
        }
    }
    return true;
}

static void dump_prop(FILE* f, const char* name, size_t k, VALUE_TYPE t, void* a, size_t n) {
    fprintf(f, "%s%zu", name, k);
    for (size_t j = 0; j < n; j++) {
        switch (t) {
            case GMTYPE_BOOL: fprintf(f, " %d", (int) ((bool*) a)[j]); break;
            case GMTYPE_INT: fprintf(f, " %d", ((int*) a)[j]); break;
            case GMTYPE_LONG: fprintf(f, " %ld", ((long*) a)[j]); break;
            case GMTYPE_FLOAT: fprintf(f, " %.9g", (double) ((float*) a)[j]); break;
            default: fprintf(f, " %.17g", ((double*) a)[j]); break;
        }
    }
    fprintf(f, "\n");
    switch (t) {
        case GMTYPE_BOOL: delete[] (bool*) a; break;
        case GMTYPE_INT: delete[] (int*) a; break;
        case GMTYPE_LONG: delete[] (long*) a; break;
        case GMTYPE_FLOAT: delete[] (float*) a; break;
        default: delete[] (double*) a; break;
    }
}

template <typename T>
static void dump_ints(FILE* f, const char* name, const T* a, size_t n) {
    fprintf(f, "%s", name);
    for (size_t j = 0; j < n; j++) fprintf(f, " %lld", (long long) a[j]);
    fprintf(f, "\n");
}

int main(int argc, char** argv) {
    if (argc < 5) {
        printf("Usage: adj_loader_check <file.adj> <vertex schema> <edge schema> <dump>\n");
        return 2;
    }
    // the tokenizer: runs of separators are one, leading and trailing ones are skipped
    GM_Tokenizer t("  12\t\t7.5 x ", " \t");
    CHECK(t.countNumberOfTokens() == 3);
    CHECK(t.hasNextToken() && t.getNextToken() == "12" && t.getNextToken() == "7.5" && t.hasNextToken() && t.getNextToken() == "x");
    CHECK(!t.hasNextToken() && t.getNextToken() == "");
    t.reset();
    CHECK(t.getNextToken() == "12");
    GM_Tokenizer tabs_only(std::string("1 2\t3"), "\t");
    CHECK(tabs_only.getNextToken() == "1 2" && tabs_only.getNextToken() == "3" && !tabs_only.hasNextToken());
    // the reader
    GM_Reader none("/nonexistent/file.adj");
    CHECK(none.failed());
    GM_Reader hdfs(argv[1], true);
    CHECK(hdfs.failed());
    GM_Reader rd(argv[1]);
    CHECK(!rd.failed());
    std::string line, first;
    long lines = 0;
    while (rd.getNextLine(line)) {
        if (lines++ == 0) first = line;
        CHECK(line.find('\n') == std::string::npos);
    }
    rd.reset();
    CHECK(rd.getNextLine(line) && line == first);

    std::vector<VALUE_TYPE> vs, es;
    CHECK(schema_of(argv[2], vs) && schema_of(argv[3], es));
    gm_graph G;
    // without a key table the keys are the ids
    CHECK(G.nodekey_to_nodeid(5) == 5 && G.nodeid_to_nodekey(7) == 7 && !G.find_nodekey(0));
    std::vector<void*> vp, ep;
    CHECK(!G.load_adjacency_list(argv[1], vs, es, vp, ep, " \t", true) && vp.empty() && ep.empty());   // HDFS: refused
    CHECK(!G.load_adjacency_list("/nonexistent/file.adj", vs, es, vp, ep, " \t") && vp.empty());
    std::vector<VALUE_TYPE> bad(1, GMTYPE_NODE);
    CHECK(!G.load_adjacency_list(argv[1], bad, es, vp, ep, " \t"));
    if (!G.load_adjacency_list(argv[1], vs, es, vp, ep, " \t")) {
        printf("load failed\n");
        return 3;
    }
    CHECK(vp.size() == vs.size() && ep.size() == es.size());
    CHECK(G.is_frozen() && G.is_semi_sorted() && G.has_reverse_edge());
    const size_t N = (size_t) G.num_nodes(), M = (size_t) G.num_edges();
    CHECK((size_t) G.get_num_nodekeys() == N);
    FILE* f = fopen(argv[4], "w");
    CHECK(f != NULL);
    fprintf(f, "N %zu\nM %zu\n", N, M);
    dump_ints(f, "begin", G.begin, N + 1);
    dump_ints(f, "node_idx", G.node_idx, M);
    dump_ints(f, "r_begin", G.r_begin, N + 1);
    dump_ints(f, "r_node_idx", G.r_node_idx, M);
    dump_ints(f, "e_idx2idx", G.e_idx2idx, M);
    fprintf(f, "keys");
    for (size_t v = 0; v < N; v++) {
        const node_t key = G.nodeid_to_nodekey((node_t) v);
        CHECK(G.find_nodekey(key) && G.nodekey_to_nodeid(key) == (node_t) v);
        fprintf(f, " %ld", (long) key);
    }
    fprintf(f, "\n");
    for (size_t k = 0; k < vs.size(); k++) dump_prop(f, "vprop", k, vs[k], vp[k], N);
    for (size_t k = 0; k < es.size(); k++) dump_prop(f, "eprop", k, es[k], ep[k], M);
    fclose(f);
    CHECK(!G.find_nodekey(-12345) && G.nodekey_to_nodeid(-12345) == gm_graph::NIL_NODE);
    // a second load replaces the first; clear_graph drops the key table
    std::vector<void*> vp2, ep2;
    CHECK(G.load_adjacency_list(argv[1], std::vector<VALUE_TYPE>(), std::vector<VALUE_TYPE>(), vp2, ep2, " \t") && vp2.empty() && ep2.empty());
    CHECK(G.num_nodes() > 0 && (size_t) G.get_num_nodekeys() == (size_t) G.num_nodes());
    G.clear_graph();
    CHECK(G.num_nodes() == 0 && G.nodekey_to_nodeid(128) == 128 && G.nodeid_to_nodekey(3) == 3 && G.get_num_nodekeys() == 0);
    // a graph built by hand has no key table either
    G.add_node();
    G.add_node();
    G.add_edge(1, 0);
    G.freeze();
    CHECK(G.nodekey_to_nodeid(1) == 1 && G.find_nodekey(1) && !G.find_nodekey(2));
    printf("adj loader ok: N = %zu, M = %zu, %ld lines\n", N, M, lines);
    return 0;
}
