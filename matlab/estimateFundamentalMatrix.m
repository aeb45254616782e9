function [F, inliersIndex, status] = estimateFundamentalMatrix(matchedPoints1, matchedPoints2, varargin)
%ESTIMATEFUNDAMENTALMATRIX libvo (MI355X) shadow: fundamental matrix of 2-D/2-D matches.
%   [F, inliersIndex, status] = estimateFundamentalMatrix(matchedPoints1, matchedPoints2, ...
%       'Method', 'MSAC', 'NumTrials', 500, 'DistanceThreshold', 0.01, 'Confidence', 99)
%   the geometric check a feature pipeline applies right after matchFeatures:
%   inliersIndex drops the stereo pairs off their epipolar line, or the
%   frame-to-frame matches that no single motion explains.  F is 3 x 3 double
%   with [x2 1] * F * [x1 1]' = 0, unit Frobenius norm, F(3, 3) >= 0.
%   Method is 'MSAC' (normalised 8-point samples, Sampson distance in squared
%   pixels, the returned F refitted over the inliers) or 'Norm8Point' (all
%   points, no sampling).  status: 0, 1 (fewer than 8 points), 2 (not enough
%   inliers); without that output the two failures are errors, as in the toolbox.
%   'RANSAC', 'LMedS', 'LTS', DistanceType 'Algebraic', InlierPercentage,
%   ReportRuntimeError and OutputClass are not implemented here: they raise
%   vo:estimateFundamentalMatrix:options -- call the toolbox's own function
%   for them (take this folder off the path around that call).
    p = inputParser;
    p.addParameter('Method', 'MSAC');
    p.addParameter('NumTrials', 500);
    p.addParameter('DistanceThreshold', 0.01);
    p.addParameter('Confidence', 99);
    p.addParameter('DistanceType', 'Sampson');
    p.KeepUnmatched = true;
    p.parse(varargin{:});
    other = fieldnames(p.Unmatched);
    if ~isempty(other)
        error('vo:estimateFundamentalMatrix:options', ...
              'estimateFundamentalMatrix: libvo does not implement the option %s; use the toolbox''s estimateFundamentalMatrix for it', other{1});
    end
    if ~strcmpi(p.Results.DistanceType, 'Sampson')
        error('vo:estimateFundamentalMatrix:options', ...
              'estimateFundamentalMatrix: libvo implements DistanceType ''Sampson'' only; use the toolbox''s estimateFundamentalMatrix for ''Algebraic''');
    end
    switch lower(char(p.Results.Method))
        case 'msac', method = 1;
        case 'norm8point', method = 0;
        otherwise
            error('vo:estimateFundamentalMatrix:options', ...
                  'estimateFundamentalMatrix: libvo implements Method ''MSAC'' and ''Norm8Point''; use the toolbox''s estimateFundamentalMatrix for ''%s''', ...
                  char(p.Results.Method));
    end
    if isobject(matchedPoints1), matchedPoints1 = matchedPoints1.Location; end
    if isobject(matchedPoints2), matchedPoints2 = matchedPoints2.Location; end
    opts = double([method, p.Results.NumTrials, p.Results.DistanceThreshold, p.Results.Confidence]);
    if nargout > 2
        [F, inliersIndex, status] = vo_mex('fundamental', matchedPoints1, matchedPoints2, opts);
    else
        [F, inliersIndex] = vo_mex('fundamental', matchedPoints1, matchedPoints2, opts);
    end
end
