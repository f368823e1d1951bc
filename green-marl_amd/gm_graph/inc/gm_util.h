// gm_util.h -- GM_Tokenizer: the tokens of a line, split at any character of a separator set; runs of separators count
// as one and leading / trailing ones are skipped (interface of the reference's apps/output_cpp/gm_graph/inc/gm_util.h:16-42).
#ifndef GM_UTIL_H_
#define GM_UTIL_H_
#include <stddef.h>
#include <string>
#include "gm_file_handling.h"

class GM_Tokenizer
{
  public:
    GM_Tokenizer(const std::string& s, const std::string& separators) : _s(s), _sep(separators), _pos(0) {}
    void setString(const std::string& s) { _s = s; _pos = 0; }
    void setDelimiter(const std::string& d) { _sep = d; _pos = 0; }
    std::string getString() { return _s; }
    std::string getDelimiter() { return _sep; }
    void reset() { _pos = 0; }
    bool hasNextToken();
    std::string getNextToken();        // "" when there is none
    long countNumberOfTokens();

  private:
    std::string _s, _sep;
    size_t _pos;   // everything before it has been handed out
};

#endif
