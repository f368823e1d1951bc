// gm_util.cc -- GM_Reader and GM_Tokenizer (clean-room; contracts in ../inc/gm_file_handling.h and ../inc/gm_util.h).
#include "gm_util.h"

#include <stdio.h>

GM_Reader::GM_Reader(const char* filename, bool hdfs) : _name(filename ? filename : ""), _failed(false) {
    if (hdfs) {
        fprintf(stderr, "GM_Reader: %s: HDFS is not supported, local files only\n", _name.c_str());
        _failed = true;
        return;
    }
    _in.open(_name.c_str(), std::ios::in | std::ios::binary);
    if (!_in.is_open()) {
        fprintf(stderr, "GM_Reader: cannot open %s\n", _name.c_str());
        _failed = true;
    }
}

void GM_Reader::reset() {
    if (_failed) return;
    _in.clear();
    _in.seekg(0, std::ios::beg);
}

bool GM_Reader::getNextLine(std::string& line) {
    if (_failed || !std::getline(_in, line)) return false;
    if (!line.empty() && line[line.size() - 1] == '\r') line.erase(line.size() - 1);
    return true;
}

int GM_Reader::readBytes(char* buf, size_t num_bytes) {
    if (_failed) return 0;
    _in.read(buf, (std::streamsize) num_bytes);
    return (int) _in.gcount();
}

void GM_Reader::terminate() {
    if (_in.is_open()) _in.close();
}

bool GM_Tokenizer::hasNextToken() { return _s.find_first_not_of(_sep, _pos) != std::string::npos; }

std::string GM_Tokenizer::getNextToken() {
    const size_t from = _s.find_first_not_of(_sep, _pos);
    if (from == std::string::npos) {
        _pos = _s.size();
        return std::string();
    }
    size_t to = _s.find_first_of(_sep, from);
    if (to == std::string::npos) to = _s.size();
    _pos = to;
    return _s.substr(from, to - from);
}

long GM_Tokenizer::countNumberOfTokens() {
    long n = 0;
    for (size_t at = _s.find_first_not_of(_sep, 0); at != std::string::npos; n++) {
        at = _s.find_first_of(_sep, at);
        if (at != std::string::npos) at = _s.find_first_not_of(_sep, at);
    }
    return n;
}
