// The one declaration of the error setter api.hip defines: records "<where>: <what>" for mmpl_last_error() (thread-local), returns 1.
#pragma once
int mmpl_set_error(const char* where, const char* what);
