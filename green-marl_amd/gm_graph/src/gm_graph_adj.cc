// gm_graph_adj.cc -- the adjacency-list text format and node keys (clean-room; contract in ../inc/gm_graph.h).
// Behavioural reference: /root/reference/apps/output_cpp/gm_graph/src/gm_graph_adj_loader.cc:20-219 (keys renumbered in
// order of appearance, destination-only keys appended in ascending order with zero values, semi-sort, reverse edges,
// edge values moved to the sorted slots through e_idx2idx) and gm_util.cc:119-179 (how a token becomes a value).
#include "gm_graph.h"

#include <stdlib.h>
#include <set>
#include <string>

#include "gm_util.h"

namespace {

// the values of one property as they are read, one vector per schema type (only the schema's is used)
struct adj_column {
    VALUE_TYPE type;
    std::vector<char> b;
    std::vector<int> i;
    std::vector<long> l;
    std::vector<float> f;
    std::vector<double> d;

    explicit adj_column(VALUE_TYPE t) : type(t) {}

    static bool supported(VALUE_TYPE t) { return t == GMTYPE_BOOL || t == GMTYPE_INT || t == GMTYPE_LONG || t == GMTYPE_FLOAT || t == GMTYPE_DOUBLE; }

    void push(const std::string& token) {
        switch (type) {
            case GMTYPE_BOOL: b.push_back(token == "true"); break;
            case GMTYPE_INT: i.push_back(atoi(token.c_str())); break;
            case GMTYPE_LONG: l.push_back(atol(token.c_str())); break;
            case GMTYPE_FLOAT: f.push_back(strtof(token.c_str(), NULL)); break;
            default: d.push_back(strtod(token.c_str(), NULL)); break;
        }
    }

    void push_zero() {
        switch (type) {
            case GMTYPE_BOOL: b.push_back(0); break;
            case GMTYPE_INT: i.push_back(0); break;
            case GMTYPE_LONG: l.push_back(0); break;
            case GMTYPE_FLOAT: f.push_back(0.0f); break;
            default: d.push_back(0.0); break;
        }
    }

    template <typename T, typename S>
    static void* gather(const std::vector<S>& src, size_t n, const edge_t* from) {
        T* out = new T[n];
        for (size_t k = 0; k < n; k++) out[k] = (T) src[from ? (size_t) from[k] : k];
        return out;
    }

    // a new[] array of n values; from != NULL: out[k] = the value read for from[k]
    void* to_array(size_t n, const edge_t* from) const {
        switch (type) {
            case GMTYPE_BOOL: return gather<bool>(b, n, from);
            case GMTYPE_INT: return gather<int>(i, n, from);
            case GMTYPE_LONG: return gather<long>(l, n, from);
            case GMTYPE_FLOAT: return gather<float>(f, n, from);
            default: return gather<double>(d, n, from);
        }
    }
};

void write_value(FILE* f, VALUE_TYPE t, const void* array, size_t k) {
    switch (t) {
        case GMTYPE_BOOL: fputs(((const bool*) array)[k] ? "true" : "false", f); break;
        case GMTYPE_INT: fprintf(f, "%d", ((const int*) array)[k]); break;
        case GMTYPE_LONG: fprintf(f, "%ld", ((const long*) array)[k]); break;
        case GMTYPE_FLOAT: fprintf(f, "%f", ((const float*) array)[k]); break;
        default: fprintf(f, "%f", ((const double*) array)[k]); break;
    }
}

bool schema_ok(const std::vector<VALUE_TYPE>& schema, const char* what) {
    for (size_t k = 0; k < schema.size(); k++)
        if (!adj_column::supported(schema[k])) {
            fprintf(stderr, "gm_graph: adjacency list: %s property %zu: type %d is not bool, int, long, float or double\n", what, k, (int) schema[k]);
            return false;
        }
    return true;
}

}   // namespace

node_t gm_graph::add_nodekey(node_t key) {
    std::unordered_map<node_t, node_t>::const_iterator it = _key2id.find(key);
    if (it != _key2id.end()) return it->second;
    const node_t id = (node_t) _id2key.size();
    _key2id[key] = id;
    _id2key.push_back(key);
    return id;
}

void gm_graph::delete_nodekey() {
    _nodekey_defined = false;
    _key2id.clear();
    std::vector<node_t>().swap(_id2key);
}

bool gm_graph::load_adjacency_list(const char* filename, std::vector<VALUE_TYPE> vprop_schema, std::vector<VALUE_TYPE> eprop_schema,
                                   std::vector<void*>& vertex_props, std::vector<void*>& edge_props, const char* separators, bool use_hdfs) {
    if (use_hdfs) {
        fprintf(stderr, "gm_graph: load_adjacency_list(%s): HDFS is not supported, local files only\n", filename);
        return false;
    }
    if (!schema_ok(vprop_schema, "vertex") || !schema_ok(eprop_schema, "edge")) return false;
    clear_graph();
    GM_Reader reader(filename, false);
    if (reader.failed()) return false;

    std::vector<adj_column> vcol, ecol;
    for (size_t k = 0; k < vprop_schema.size(); k++) vcol.push_back(adj_column(vprop_schema[k]));
    for (size_t k = 0; k < eprop_schema.size(); k++) ecol.push_back(adj_column(eprop_schema[k]));
    std::vector<edge_t> row_begin;   // of the sources, in file order
    std::vector<node_t> dest;        // destination KEYS, in file order
    _nodekey_defined = true;
    std::string line;
    long line_no = 0;
    while (reader.getNextLine(line)) {
        line_no++;
        GM_Tokenizer tok(line, separators);
        if (!tok.hasNextToken()) continue;
        const node_t key = (node_t) atol(tok.getNextToken().c_str());
        if (_key2id.count(key)) {
            fprintf(stderr, "gm_graph: %s:%ld: key %ld starts a second line\n", filename, line_no, (long) key);
            clear_graph();
            return false;
        }
        add_nodekey(key);
        row_begin.push_back((edge_t) dest.size());
        bool whole = true;
        for (size_t k = 0; k < vcol.size() && whole; k++) {
            whole = tok.hasNextToken();
            if (whole) vcol[k].push(tok.getNextToken());
        }
        while (whole && tok.hasNextToken()) {
            dest.push_back((node_t) atol(tok.getNextToken().c_str()));
            for (size_t k = 0; k < ecol.size() && whole; k++) {
                whole = tok.hasNextToken();
                if (whole) ecol[k].push(tok.getNextToken());
            }
        }
        if (!whole) {
            fprintf(stderr, "gm_graph: %s:%ld: the line ends inside the values of a vertex or an edge\n", filename, line_no);
            clear_graph();
            return false;
        }
    }
    const edge_t M = (edge_t) dest.size();
    // keys that are only ever destinations: after the sources, ascending, with zero values and no out-edges
    std::set<node_t> dest_only;
    for (size_t e = 0; e < dest.size(); e++)
        if (!_key2id.count(dest[e])) dest_only.insert(dest[e]);
    for (std::set<node_t>::const_iterator it = dest_only.begin(); it != dest_only.end(); ++it) {
        add_nodekey(*it);
        row_begin.push_back(M);
        for (size_t k = 0; k < vcol.size(); k++) vcol[k].push_zero();
    }
    row_begin.push_back(M);
    const node_t N = (node_t) _id2key.size();

    prepare_external_creation(N, M, false);   // (keeps the key table)
    for (node_t v = 0; v <= N; v++) begin[v] = row_begin[(size_t) v];
    for (edge_t e = 0; e < M; e++) node_idx[e] = _key2id[dest[(size_t) e]];
    do_semi_sort();          // e_idx2idx[slot] = the slot's place in the file
    make_reverse_edges();
    for (size_t k = 0; k < vcol.size(); k++) vertex_props.push_back(vcol[k].to_array((size_t) N, NULL));
    for (size_t k = 0; k < ecol.size(); k++) edge_props.push_back(ecol[k].to_array((size_t) M, e_idx2idx));
    return true;
}

bool gm_graph::store_adjacency_list(const char* filename, std::vector<VALUE_TYPE> vprop_schema, std::vector<VALUE_TYPE> eprop_schema,
                                    std::vector<void*>& vertex_props, std::vector<void*>& edge_props, const char* separators, bool use_hdfs) {
    if (use_hdfs) {
        fprintf(stderr, "gm_graph: store_adjacency_list(%s): HDFS is not supported, local files only\n", filename);
        return false;
    }
    if (!schema_ok(vprop_schema, "vertex") || !schema_ok(eprop_schema, "edge")) return false;
    if (vertex_props.size() < vprop_schema.size() || edge_props.size() < eprop_schema.size()) return false;
    if (!_frozen) freeze();
    FILE* f = fopen(filename, "w");
    if (f == NULL) {
        fprintf(stderr, "gm_graph: cannot open %s for writing\n", filename);
        return false;
    }
    for (node_t v = 0; v < _numNodes; v++) {
        fprintf(f, "%ld", (long) nodeid_to_nodekey(v));
        for (size_t k = 0; k < vprop_schema.size(); k++) {
            fputs(separators, f);
            write_value(f, vprop_schema[k], vertex_props[k], (size_t) v);
        }
        for (edge_t e = begin[v]; e < begin[v + 1]; e++) {
            fputs(separators, f);
            fprintf(f, "%ld", (long) nodeid_to_nodekey(node_idx[e]));
            for (size_t k = 0; k < eprop_schema.size(); k++) {
                fputs(separators, f);
                write_value(f, eprop_schema[k], edge_props[k], (size_t) e);
            }
        }
        fputc('\n', f);
    }
    return fclose(f) == 0;
}
