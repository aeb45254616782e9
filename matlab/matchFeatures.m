function [indexPairs, matchMetric] = matchFeatures(features1, features2, varargin)
%MATCHFEATURES libvo (MI355X) shadow: [indexPairs, matchMetric] = matchFeatures(features1, features2, Name, Value)
%   reference call sites: VO.m:87,283,293,311,323.  Exhaustive, SSD; options
%   'Unique' (the toolbox's findUniqueIndices rule), 'MatchThreshold' (percent,
%   (0, 25]: libvo stops where the SSD threshold reaches 1) and 'MaxRatio'
%   ((0, 1]); 'Method', 'Metric' and 'Prenormalized' only at their defaults.
%   Anything else raises vo:matchFeatures:options (the gateway parses them).
%   The N x 128 single descriptors are handed over as they lie (column-major,
%   no conversion on the host); indexPairs is P x 2 uint32, ascending in the
%   first column; matchMetric is P x 1 single, the SSD of each pair.
%   u8-valued rows (extractFeatures' SIFT descriptors, all VO.m passes) take
%   libvo's exact-integer path; any other single features take its float SSD
%   path (rows normalised to unit length, SSD summed in a fixed order).
    if nargout > 1
        [indexPairs, matchMetric] = vo_mex('match', single(features1), single(features2), varargin{:});
    else
        indexPairs = vo_mex('match', single(features1), single(features2), varargin{:});
    end
end
