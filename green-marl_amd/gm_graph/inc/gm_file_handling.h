// gm_file_handling.h -- GM_Reader: a text file, one line at a time (what gm_graph::load_adjacency_list and a driver that
// reads a config file use; interface of the reference's apps/output_cpp/gm_graph/inc/gm_file_handling.h:37-67).  Local
// files only: a reader asked for HDFS fails, with a message.
#ifndef GM_FILE_HANDLING_H_
#define GM_FILE_HANDLING_H_
#include <stddef.h>
#include <fstream>
#include <string>

class GM_Reader
{
  public:
    GM_Reader(const char* filename, bool hdfs = false);
    bool failed() { return _failed; }
    void reset();                             // back to the first line
    bool getNextLine(std::string& line);      // false at the end of the file; the line comes without its '\n' (and '\r')
    int readBytes(char* buf, size_t num_bytes);
    void terminate();

  private:
    std::string _name;
    std::ifstream _in;
    bool _failed;
};

#endif
