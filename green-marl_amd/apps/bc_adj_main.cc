// bc_adj_main.cc -- exact betweenness centrality of an adjacency-list graph: comp_BC(G, BC) of bc_adj.gm, then the BC of
// the vertices a config file asks for.  The command line and the output lines are those of the reference's driver
// (apps/output_cpp/src/bc_adj_main.cc):
//     bc_adj <input.adj> <config_file> <num_threads> [edge_values]
// The first line of the config file lists the keys to print.  A line of the input is `key value [dst-key values]*`: one
// double per vertex and, per edge, the values `edge_values` names -- d = a double, l = a long; the default "dl" is the
// reference driver's schema (a cost and an edge key), "d" reads the reference's small sample files.
#include <assert.h>
#include <sys/time.h>

#include <string>

#include "bc_adj.h"
#include "gm.h"
#include "gm_file_handling.h"
#include "gm_util.h"

int main(int argc, char** argv) {
    if (argc < 4) {
        printf("Usage: ./bc_adj <input_file> <config_file> <num_threads> [edge_values: d | l ...]\n");
        exit(1);
    }
    const char* input = argv[1];
    const char* config = argv[2];
    const int num = atoi(argv[3]);
    printf("running with %d threads\n", num);
    gm_rt_set_num_threads(num);

    std::vector<VALUE_TYPE> vprop_schema(1, GMTYPE_DOUBLE), eprop_schema;
    for (const char* c = argc > 4 ? argv[4] : "dl"; *c; c++) {
        if (*c != 'd' && *c != 'l') {
            printf("edge_values: d (a double) or l (a long) per edge value\n");
            exit(1);
        }
        eprop_schema.push_back(*c == 'd' ? GMTYPE_DOUBLE : GMTYPE_LONG);
    }
    gm_graph G;
    std::vector<void*> vertex_props, edge_props;
    if (!G.load_adjacency_list(input, vprop_schema, eprop_schema, vertex_props, edge_props, " \t", false)) {
        printf("cannot load %s\n", input);
        exit(1);
    }

    const char* separators = " \t";
    GM_Reader reader(config, false);
    if (reader.failed()) exit(1);
    std::string line;
    gm_node_seq Outputs;
    if (reader.getNextLine(line)) {
        GM_Tokenizer tok(line, separators);
        while (tok.hasNextToken()) {
            const node_t key = (node_t) atol(tok.getNextToken().c_str());
            if (!G.find_nodekey(key)) {
                printf("%ld is not a key of %s\n", (long) key, input);
                exit(1);
            }
            Outputs.push_back(G.nodekey_to_nodeid(key));
        }
    }

    float* BC = new float[(size_t) G.num_nodes() + 1];
    struct timeval T1, T2;
    gettimeofday(&T1, NULL);
    comp_BC(G, BC);
    gettimeofday(&T2, NULL);
    printf("BC (threads: %d) - COMPUTATION RUNNING TIME (ms): %lf\n", num, (T2.tv_sec - T1.tv_sec) * 1000 + (T2.tv_usec - T1.tv_usec) * 0.001);

    gm_node_seq::seq_iter it = Outputs.prepare_seq_iteration();
    while (it.has_next()) {
        const node_t n = it.get_next();
        printf("%d :  %f\n", (int) G.nodeid_to_nodekey(n), BC[n]);
    }
    printf("\n");
    delete[] BC;
    delete[] (double*) vertex_props[0];
    for (size_t k = 0; k < edge_props.size(); k++) {
        if (eprop_schema[k] == GMTYPE_DOUBLE) delete[] (double*) edge_props[k];
        else delete[] (long*) edge_props[k];
    }
    return 0;
}
